// Host trace of the TGN step: what csrc/tgn.hip QUEUES, without a GPU.
//
// tgn.hip holds no kernel, so `hipcc --cuda-host-only -c tgn.hip` is a plain host object.  This program defines every symbol
// that object leaves undefined - the eight HIP calls it makes and the launchers, size queries and hooks of gemm.hpp, attn.hpp,
// memory.hpp and common.hpp - as RECORDERS, links against that one object and drives the C ABI through a fixed list of
// scenarios.  Every call becomes one text line: name, stream, every argument, every field of a descriptor.  Pointers are
// written as region+offset: the scenario hands in fake, non-null bases that nothing here or in tgn.hip dereferences.
//
//   step_trace OUTDIR      writes OUTDIR/<scenario>.log, prints "<scenario> <rc>" per scenario, exits 1 if any rc != PFO_OK
//
// Two versions of tgn.hip queue the same step iff their logs are byte-identical (tests/test_step_trace_cpu.py).
#include "gemm.hpp"
#include "attn.hpp"
#include "memory.hpp"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

int pfo_tnbr_sample_dev(const int64_t*, const int32_t*, const int32_t*, const double*, int64_t, const int32_t*, const double*,
                        int64_t, int32_t, int32_t, const int64_t*, uint64_t, uint64_t, const uint64_t*, int32_t*, int32_t*,
                        float*, float*, int32_t*, double*, int32_t*, int32_t*, void*, int32_t*, int64_t);
int pfo_adam_step_ranges_impl(float*, float*, float*, float*, int32_t, const int64_t*, const int64_t*, const int32_t*, float, float,
                              float, float, bool, void*);

namespace {

// ---- what a scenario sets for the stubs
struct Knobs {
  bool uses_runs = true, runs_possible = true, needs_winner = false, prof = false, marks = false;
  hipStream_t capturing = nullptr;   // the stream that reports an active capture
  int n_parts = 0;                   // pfo_attn_bwd_launch's *n_parts; 0: the slab rows of a deterministic launch, else the bins
};
Knobs K;
FILE* out = nullptr;
std::string last_error;

// ---- names: regions, streams, events
struct Region { const char* name; uintptr_t base; };
const uintptr_t REGION_SPAN = (uintptr_t)1 << 36;            // 64 GiB apart: an offset never reaches the next base
std::vector<Region> regions;
void* region(const char* name) {
  for (const Region& r : regions) if (!strcmp(r.name, name)) return (void*)r.base;
  regions.push_back({name, REGION_SPAN * (regions.size() + 16)});
  return (void*)regions.back().base;
}
template <typename T> T* reg(const char* name) { return reinterpret_cast<T*>(region(name)); }

std::string ptr_name(const void* p) {
  if (!p) return "null";
  const uintptr_t v = (uintptr_t)p;
  for (const Region& r : regions)
    if (v >= r.base && v < r.base + REGION_SPAN) return std::string(r.name) + "+" + std::to_string(v - r.base);
  return "UNKNOWN";                                           // a pointer no scenario handed in: a host address would not repeat
}

// Streams and events are handles the program makes up.  The library's own are named in order of creation: the table follows
// side() in tgn.hip (an event created beyond it is ev<k>); the caller's get the name the scenario gives them.
const char* const SIDE_STREAMS[] = {"side1", "side2"};
const char* const SIDE_EVENTS[] = {"tn_a_done", "done2", "fork", "done", "seg_done", "tn_a", "tn_b", "fold_done", "gru_done",
                                   "comp_done", "pc_a", "pc_b", "main_done", "side_done", "early_done",
                                   "layer[0]", "layer[1]", "layer[2]", "layer[3]", "layer[4]"};
std::vector<std::string> stream_names, event_names;
int n_lib_streams = 0, n_lib_events = 0;
const uintptr_t STREAM_BASE = (uintptr_t)1 << 32, EVENT_BASE = (uintptr_t)2 << 32;
hipStream_t new_stream(const std::string& name) {
  stream_names.push_back(name);
  return (hipStream_t)(STREAM_BASE + 64 * stream_names.size());
}
hipEvent_t new_event(const std::string& name) {
  event_names.push_back(name);
  return (hipEvent_t)(EVENT_BASE + 64 * event_names.size());
}
std::string stream_name(const void* s) {
  if (!s) return "null";
  const uintptr_t i = ((uintptr_t)s - STREAM_BASE) / 64;
  return (i >= 1 && i <= stream_names.size()) ? stream_names[i - 1] : "UNKNOWN";
}
std::string event_name(const void* e) {
  if (!e) return "null";
  const uintptr_t i = ((uintptr_t)e - EVENT_BASE) / 64;
  return (i >= 1 && i <= event_names.size()) ? event_names[i - 1] : "UNKNOWN";
}

// ---- one log line
struct Line {
  explicit Line(const char* what) { fputs(what, out); }
  ~Line() { fputc('\n', out); }
  Line& on(const void* stream) { fprintf(out, " stream=%s", stream_name(stream).c_str()); return *this; }
  Line& ev(const char* k, const void* e) { fprintf(out, " %s=%s", k, event_name(e).c_str()); return *this; }
  Line& p(const char* k, const void* v) { fprintf(out, " %s=%s", k, ptr_name(v).c_str()); return *this; }
  Line& i(const char* k, long long v) { fprintf(out, " %s=%lld", k, v); return *this; }
  Line& u(const char* k, unsigned long long v) { fprintf(out, " %s=%llu", k, v); return *this; }
  Line& f(const char* k, double v) { fprintf(out, " %s=%.9g", k, v); return *this; }
  Line& s(const char* k, const char* v) { fprintf(out, " %s=\"%s\"", k, v); return *this; }
};
#define FI(x) ln.i(#x, (long long)(d.x))
#define FP(x) ln.p(#x, d.x)

void log_gemm(const char* what, const PfoGemm& d, int index, hipStream_t stream) {
  Line ln(what);
  ln.on(stream).i("i", index);
  for (int q = 0; q < 2; ++q) {
    const std::string t = std::to_string(q);
    ln.p(("A" + t).c_str(), d.A[q]).i(("lda" + t).c_str(), d.lda[q]).p(("a_idx" + t).c_str(), d.a_idx[q]);
    ln.p(("B" + t).c_str(), d.B[q]).i(("ldb" + t).c_str(), d.ldb[q]).i(("K" + t).c_str(), d.K[q]);
    ln.i(("a_bs" + t).c_str(), d.a_bs[q]).i(("b_bs" + t).c_str(), d.b_bs[q]);
  }
  FP(b_idx); FP(C); FI(ldc); FP(bias); FP(row_scale); FI(rs_ld); FP(row_zero); FP(relu_src); FI(relu_ld);
  FP(add_src); FI(add_ld); FP(add_idx); FI(M); FI(N); FP(m_dev); FI(relu); FI(accumulate); FI(a_kmajor); FI(b_kmajor);
  FI(batch); FI(c_bs); FI(bias_bs); FI(rs_bs); FP(slabs); FI(slab_floats); FP(b_img); FP(b_img2); FI(bx_force);
}
void log_attn(const char* what, const PfoAttn& d, hipStream_t stream) {
  Line ln(what);
  ln.on(stream);
  FI(N); FI(K); FI(D); FI(Ef); FI(H); FI(Cp); FP(QK); FP(qk_row); FI(qk_ld); FP(nbr_tab); FI(nbr_ld); FP(nbr_row);
  FI(nbr_row_base); FI(nbr_rows); FI(edge_rows); FI(nbr_relu); FP(nbr_ids); FP(edge_feat); FP(eidx); FP(dt); FP(tw); FP(tb);
  ln.f("scale", d.scale).f("dropout_p", d.dropout_p).u("seed", d.seed).u("offset", d.offset);
  FP(offset_dev); FP(keep_inject); FP(ctx); FP(attw); FP(inv); FP(dctx); FP(dQK); FP(d_nbr); FI(d_nbr_ld); FI(d_nbr_rep);
  FI(d_nbr_nrep); FP(dtime_part); FI(det); FP(dtime_slab); FP(dqk_live); FP(members); FP(seg_ptr); FP(n_rows); FP(run_cnt);
}

}  // namespace

// =============================================================================================
// The eight HIP calls.  hipStreamIsCapturing is a query, not an action: it is answered and not logged.
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int flags, int priority) {
  const int k = n_lib_streams++;
  *s = new_stream(k < 2 ? SIDE_STREAMS[k] : "stream" + std::to_string(k));
  Line("hipStreamCreateWithPriority").on(*s).u("flags", flags).i("priority", priority);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  const int k = n_lib_events++;
  *e = new_event(k < (int)(sizeof(SIDE_EVENTS) / sizeof(SIDE_EVENTS[0])) ? SIDE_EVENTS[k] : "ev" + std::to_string(k));
  Line("hipEventCreateWithFlags").ev("event", *e).u("flags", flags);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { Line("record").on(s).ev("event", e); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int flags) {
  Line("wait").on(s).ev("event", e).u("flags", flags);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
  Line("memset").on(s).p("dst", dst).i("value", value).u("bytes", bytes);
  return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus* status) {
  *status = (K.capturing && s == K.capturing) ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  return hipSuccess;
}

// ---- common.hpp
void pfo_set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error = buf;
}
bool pfo_prof_on() { return K.prof; }
bool pfo_marks_on() { return K.marks; }
void pfo_mark_at(const char* name, hipStream_t s) { Line("mark").on(s).s("name", name); }
void pfo_range_push(const char* name) { Line("range_push").s("name", name); }
void pfo_range_pop() { Line("range_pop"); }
void pfo_stop_event_arm(hipEvent_t e, int skip) { Line("arm").ev("event", e).i("skip", skip); }
void pfo_stop_event_disarm(hipStream_t s) { Line("disarm").on(s); }
void pfo_stop_event_cancel() { Line("cancel"); }

// ---- size and path queries: fixed formulas (two versions of tgn.hip see the same ones), branches set per scenario
int64_t pfo_bimg_bytes(int N, int K_) { return (int64_t)N * K_ * 6 + 1024; }
int64_t pfo_gru_img_bytes(int D, int K_) { return (int64_t)4 * D * K_ * 6 + 1024; }
int64_t pfo_seg_of_ints(int64_t n) { return n + 64; }
int64_t pfo_seg_scratch_ints(int cap) { return (int64_t)cap + 1024; }
int64_t pfo_compact_scratch_ints(int n) { return 2 * (int64_t)n / 1024 + 64; }
int64_t pfo_fold_parts_scratch_doubles(int n) { return (int64_t)64 * n; }
int64_t pfo_attn_bwd_det_parts(int64_t N) { return (N + 63) / 64; }
int pfo_attn_bwd_max_parts() { return ATTN_TIME_BINS; }
bool pfo_attn_bwd_uses_runs(const PfoAttn& a) { return K.uses_runs && a.members != nullptr; }
bool pfo_attn_bwd_runs_possible(int, int, int) { return K.runs_possible; }
bool pfo_msg_store_needs_winner(int) { return K.needs_winner; }

// ---- gemm.hpp
int pfo_gemm_launch(const PfoGemm& g, hipStream_t s) { log_gemm("pfo_gemm_launch", g, 0, s); return PFO_OK; }
int pfo_gemm_multi_launch(const PfoGemm* list, int n, hipStream_t s) {
  Line("pfo_gemm_multi_launch").on(s).i("n", n);
  for (int i = 0; i < n; ++i) log_gemm("  gemm", list[i], i, s);
  return PFO_OK;
}
int pfo_bimg_launch(const PfoBimg* list, int n, hipStream_t s) {
  Line("pfo_bimg_launch").on(s).i("n", n);
  for (int i = 0; i < n; ++i) {
    const PfoBimg& d = list[i];
    Line ln("  bimg");
    ln.i("i", i);
    FP(src); FI(ld); FI(N); FI(K); FI(trans); FP(dst); FI(row0); FI(rows_total); FI(last); FI(gate); FI(gate_D);
  }
  return PFO_OK;
}
int pfo_gru_fused_launch(const PfoGruFused& d, hipStream_t s) {
  Line ln("pfo_gru_fused_launch");
  ln.on(s);
  FP(msg_rows); FI(K_msg); FP(h_rows); FP(img_ih); FP(img_hh); FP(b_ih); FP(b_hh); FP(hm); FP(touched); FP(node_feat);
  FP(upd_mem); FP(h0_tab); FP(gates); FI(D); FI(cap_rows); FP(n_rows); FI(gather);
  return PFO_OK;
}
int pfo_rank1_multi_launch(const PfoRank1* list, int n, hipStream_t s) {
  Line("pfo_rank1_multi_launch").on(s).i("n", n);
  for (int i = 0; i < n; ++i) {
    const PfoRank1& d = list[i];
    Line ln("  rank1");
    ln.i("i", i);
    FP(u); FI(ldu); FP(v); FI(ldv); FI(M); FI(N); FP(out); FI(ldo); FI(reps); FI(u_rs); FI(v_rs);
  }
  return PFO_OK;
}
int pfo_sum_slabs_launch(const PfoSumSlabs* list, int n, hipStream_t s) {
  Line("pfo_sum_slabs_launch").on(s).i("n", n);
  for (int i = 0; i < n; ++i) {
    const PfoSumSlabs& d = list[i];
    Line ln("  sum_slabs");
    ln.i("i", i);
    FP(dst); FP(src); FI(stride); FI(count); FI(n_slabs); FI(accumulate);
  }
  return PFO_OK;
}
int pfo_gemm_tn_group_launch(const PfoTnProblem* probs, int n, int K_, const int32_t* k_dev, float* slabs, int64_t slab_floats,
                             hipStream_t s) {
  Line("pfo_gemm_tn_group_launch").on(s).i("n", n).i("K", K_).p("k_dev", k_dev).p("slabs", slabs).i("slab_floats", slab_floats);
  for (int i = 0; i < n; ++i) {
    const PfoTnProblem& d = probs[i];
    Line ln("  tn");
    ln.i("i", i);
    FP(A); FI(lda); FP(B); FI(ldb); FP(b_idx); FI(M); FI(N); FP(C); FI(ldc); FI(c_accumulate); FP(bias_out); FI(bias_accumulate);
  }
  return PFO_OK;
}

// ---- attn.hpp
int pfo_attn_fwd_launch(const PfoAttn& a, hipStream_t s) { log_attn("pfo_attn_fwd_launch", a, s); return PFO_OK; }
int pfo_attn_bwd_launch(const PfoAttn& a, int* n_parts, hipStream_t s) {
  log_attn("pfo_attn_bwd_launch", a, s);
  *n_parts = K.n_parts ? K.n_parts : (a.det ? (int)pfo_attn_bwd_det_parts(a.N) : ATTN_TIME_BINS);
  return PFO_OK;
}

// ---- memory.hpp, the sampler, the time encoder, the optimizer
int pfo_touch_compact_launch(const int32_t* nodes0, int64_t n0, const int32_t* extra, int64_t n_extra, int n_nodes, int32_t* mark,
                             int32_t* slot, int32_t* touched_ids, int32_t* n_counts, int32_t* scratch, bool marks_are_zero,
                             bool marked, hipStream_t s) {
  Line("pfo_touch_compact_launch").on(s).p("nodes0", nodes0).i("n0", n0).p("extra", extra).i("n_extra", n_extra)
      .i("n_nodes", n_nodes).p("mark", mark).p("slot", slot).p("touched_ids", touched_ids).p("n_counts", n_counts)
      .p("scratch", scratch).i("marks_are_zero", marks_are_zero).i("marked", marked);
  return PFO_OK;
}
int pfo_pack_remap_launch(const float* msg_table, int M, const float* memory, int D, const uint8_t* has_msg,
                          const int32_t* touched_ids, const int32_t* n_touched, int cap, float* msg_rows, float* h_rows,
                          uint8_t* hm, const int32_t* nodes0, int64_t n0, const int32_t* slot, int32_t* idx0, hipStream_t s) {
  Line("pfo_pack_remap_launch").on(s).p("msg_table", msg_table).i("M", M).p("memory", memory).i("D", D).p("has_msg", has_msg)
      .p("touched_ids", touched_ids).p("n_touched", n_touched).i("cap", cap).p("msg_rows", msg_rows).p("h_rows", h_rows)
      .p("hm", hm).p("nodes0", nodes0).i("n0", n0).p("slot", slot).p("idx0", idx0);
  return PFO_OK;
}
int pfo_gru_gates_bwd_launch(const float* gates, float* dgi, float* dgh, const float* h_rows, const uint8_t* hm,
                             const int32_t* n_touched, int cap, int D, const float* d_h0, int n_rep, int64_t rep_stride,
                             const float* d_extra, int det, hipStream_t s) {
  Line("pfo_gru_gates_bwd_launch").on(s).p("gates", gates).p("dgi", dgi).p("dgh", dgh).p("h_rows", h_rows).p("hm", hm)
      .p("n_touched", n_touched).i("cap", cap).i("D", D).p("d_h0", d_h0).i("n_rep", n_rep).i("rep_stride", rep_stride)
      .p("d_extra", d_extra).i("det", det);
  return PFO_OK;
}
int pfo_seg_build_launch(const int32_t* idx, const int32_t* nodes, int N, int cap_rows, const int32_t* key_src, int32_t* seg_ptr,
                         int32_t* cursor, int32_t* tmp, int32_t* members, int32_t* seg_of, int32_t* scratch, hipStream_t s) {
  Line("pfo_seg_build_launch").on(s).p("idx", idx).p("nodes", nodes).i("N", N).i("cap_rows", cap_rows).p("key_src", key_src)
      .p("seg_ptr", seg_ptr).p("cursor", cursor).p("tmp", tmp).p("members", members).p("seg_of", seg_of).p("scratch", scratch);
  return PFO_OK;
}
int pfo_segsum_launch(const float* src0, int W0, const float* src1, int W1, const int32_t* seg_ptr, const int32_t* members,
                      const int32_t* seg_of, int64_t cap_members, const int32_t* n_rows, int cap_rows, int src0_by_position,
                      const uint8_t* src0_live, float* out_, hipStream_t s) {
  Line("pfo_segsum_launch").on(s).p("src0", src0).i("W0", W0).p("src1", src1).i("W1", W1).p("seg_ptr", seg_ptr)
      .p("members", members).p("seg_of", seg_of).i("cap_members", cap_members).p("n_rows", n_rows).i("cap_rows", cap_rows)
      .i("src0_by_position", src0_by_position).p("src0_live", src0_live).p("out", out_);
  return PFO_OK;
}
int pfo_zero_rows_launch(float* dst, const int32_t* n_rows, int cap_rows, int D, int n_rep, int64_t rep_stride, hipStream_t s) {
  Line("pfo_zero_rows_launch").on(s).p("dst", dst).p("n_rows", n_rows).i("cap_rows", cap_rows).i("D", D).i("n_rep", n_rep)
      .i("rep_stride", rep_stride);
  return PFO_OK;
}
int pfo_persist_launch(const int32_t* src, const int32_t* dst, int B, const int32_t* slot, const float* upd_mem,
                       const uint8_t* has_msg, const float* msg_time, float* memory, float* last_update, int D, int32_t* winner,
                       hipStream_t s) {
  Line("pfo_persist_launch").on(s).p("src", src).p("dst", dst).i("B", B).p("slot", slot).p("upd_mem", upd_mem)
      .p("has_msg", has_msg).p("msg_time", msg_time).p("memory", memory).p("last_update", last_update).i("D", D)
      .p("winner", winner);
  return PFO_OK;
}
int pfo_msg_store_launch(const int32_t* src, const int32_t* dst, const double* ts, const int32_t* eidx, int B, const float* memory,
                         const float* last_update, const float* edge_feat, const float* tw, const float* tb, int D, int Ef,
                         float* msg_table, float* msg_time, uint8_t* has_msg, int32_t* winner, hipStream_t s) {
  Line("pfo_msg_store_launch").on(s).p("src", src).p("dst", dst).p("ts", ts).p("eidx", eidx).i("B", B).p("memory", memory)
      .p("last_update", last_update).p("edge_feat", edge_feat).p("tw", tw).p("tb", tb).i("D", D).i("Ef", Ef)
      .p("msg_table", msg_table).p("msg_time", msg_time).p("has_msg", has_msg).p("winner", winner);
  return PFO_OK;
}
int pfo_observe_select_launch(const int32_t* src, const int32_t* dst, int B, const uint8_t* has_msg, int32_t* rep, int base,
                              int32_t* slot, int32_t* touched, int32_t* n_out, hipStream_t s) {
  Line("pfo_observe_select_launch").on(s).p("src", src).p("dst", dst).i("B", B).p("has_msg", has_msg).p("rep", rep)
      .i("base", base).p("slot", slot).p("touched", touched).p("n_out", n_out);
  return PFO_OK;
}
int pfo_mean_launch(const float* src, int64_t n, float* out_, hipStream_t s) {
  Line("pfo_mean_launch").on(s).p("src", src).i("n", n).p("out", out_);
  return PFO_OK;
}
int pfo_cq_backward_launch(const float* const* gq, const float* const* Wq, int n_layers, const float* tb, int D, float* const* d_bq,
                           float* const* d_Wq, float* d_tb, float* tb_part, const float* tb_add, const double* dtime, int n_bins,
                           float* d_tw, hipStream_t s) {
  Line ln("pfo_cq_backward_launch");
  ln.on(s).i("n_layers", n_layers);
  for (int l = 0; l < n_layers; ++l) {                          // host arrays of device pointers: element by element
    const std::string t = std::to_string(l);
    ln.p(("gq" + t).c_str(), gq[l]).p(("Wq" + t).c_str(), Wq[l]).p(("d_bq" + t).c_str(), d_bq[l]).p(("d_Wq" + t).c_str(), d_Wq[l]);
  }
  ln.p("tb", tb).i("D", D).p("d_tb", d_tb).p("tb_part", tb_part).p("tb_add", tb_add).p("dtime", dtime).i("n_bins", n_bins)
      .p("d_tw", d_tw);
  return PFO_OK;
}
int pfo_fold_parts_launch(const double* parts, int n_parts, int n, float* out_, int accumulate, double* scratch, int* tickets,
                          hipStream_t s, double* out64) {
  Line("pfo_fold_parts_launch").on(s).p("parts", parts).i("n_parts", n_parts).i("n", n).p("out", out_).i("accumulate", accumulate)
      .p("scratch", scratch).p("tickets", tickets).p("out64", out64);
  return PFO_OK;
}
int pfo_tnbr_sample_dev(const int64_t* indptr, const int32_t* adj_nbr, const int32_t* adj_eidx, const double* adj_ts,
                        int64_t n_nodes, const int32_t* nodes, const double* ts, int64_t n, int32_t Kn, int32_t uniform,
                        const int64_t* draws, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int32_t* out_nbr,
                        int32_t* out_eidx, float* out_ts, float* out_dt, int32_t* next_nodes, double* next_ts, int32_t* mark,
                        int32_t* cnt, void* stream, int32_t* clear, int64_t clear_n) {
  Line("pfo_tnbr_sample_dev").on(stream).p("indptr", indptr).p("adj_nbr", adj_nbr).p("adj_eidx", adj_eidx).p("adj_ts", adj_ts)
      .i("n_nodes", n_nodes).p("nodes", nodes).p("ts", ts).i("n", n).i("K", Kn).i("uniform", uniform).p("draws", draws)
      .u("seed", seed).u("offset", offset).p("offset_dev", offset_dev).p("out_nbr", out_nbr).p("out_eidx", out_eidx)
      .p("out_ts", out_ts).p("out_dt", out_dt).p("next_nodes", next_nodes).p("next_ts", next_ts).p("mark", mark).p("cnt", cnt)
      .p("clear", clear).i("clear_n", clear_n);
  return PFO_OK;
}
extern "C" int pfo_time_encode(const float* t, int64_t n, const float* w, const float* b, int32_t D, float* out_, void* stream) {
  Line("pfo_time_encode").on(stream).p("t", t).i("n", n).p("w", w).p("b", b).i("D", D).p("out", out_);
  return PFO_OK;
}
int pfo_adam_step_ranges_impl(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges, const int64_t* lo,
                              const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2, float eps,
                              bool zero_grad, void* stream) {
  Line("pfo_adam_step_ranges_impl").on(stream).p("param", param).p("grad", grad).p("exp_avg", exp_avg).p("exp_avg_sq", exp_avg_sq)
      .i("n_ranges", n_ranges).p("lo", lo).p("hi", hi).p("step", step).f("lr", lr).f("beta1", beta1).f("beta2", beta2)
      .f("eps", eps).i("zero_grad", zero_grad);
  return PFO_OK;
}

// =============================================================================================
// Scenarios.  One scenario = a sequence of ABI calls as a caller would make them, in one process with the others (the side
// streams, their events and the deferred-work generations of tgn.hip are static and carry over), closed by pfo_tgn_join on
// the caller's stream.  Where a CALLER has to order two of its own streams (a prepared batch, a forward that moved to another
// stream) the scenario records and waits for an event of its own, as that caller would.
namespace {

struct Scn {
  const char* name;
  int L = 2, mem = 1, uniform = 0, det = 0, prof = 0, marks = 0, capture = 0;
  int pcache = 0;        // 0 none, 1 valid, 2 given but invalid, 3 valid after pfo_tgn_refresh
  int prepared = 0;      // pfo_tgn_prepare on the second caller's stream, then a prepared forward
  int fused = 0;         // 0: pfo_tgn_update_state after the forward, 1: upd_* in the forward, 2: + seg_in_forward
  int defer = 0;         // defer_join, then 1: pfo_tgn_adam_side, 2: pfo_tgn_adam_side_bucket (first use, then later bucket),
                         // 3: no optimizer step behind it, 4: one plain bucket (flags 0)
  int next_fwd = 0;      // after the step, a second step's forward: 1 on the same stream, 2 on the other
  int mid = 0;           // mid_event: 1 early, 2 late
  int top_ready = 0, mean = 0, zero_grad = 0, n_extra = 0, keep = 0;
  int observe = 0;       // pfo_tgn_observe alone: 1 a short log, 2 one long enough for the stamp table to start over
  int eval = 0;          // training = 0: the forward alone
  int uses_runs = 1, runs_possible = 1, needs_winner = 0;
  int n_nodes = 50000;   // (small graphs: the upper level's sampler launch clears the compaction's flags - prepare_sample)
  float dropout = 0.f;
};

struct Run {
  const Scn& sc;
  pfo_tgn_config c;
  pfo_tgn_state st;
  pfo_tgn_batch b;
  hipStream_t main_s, other_s;
  const int64_t* draws[PFO_MAX_LAYERS];
  const uint8_t* keeps[PFO_MAX_LAYERS];
  void* ws;
  explicit Run(const Scn& s) : sc(s) {
    memset(&c, 0, sizeof(c)); memset(&st, 0, sizeof(st)); memset(&b, 0, sizeof(b));
    c.n_nodes = sc.n_nodes; c.n_edges_p1 = 20001; c.D = 32; c.Ef = 16; c.n_layers = sc.L; c.n_heads = 2; c.use_memory = sc.mem;
    c.max_roots = 96; c.max_neighbors = 10; c.max_batch = 32;
    st.indptr = reg<int64_t>("indptr"); st.adj_nbr = reg<int32_t>("adj_nbr"); st.adj_eidx = reg<int32_t>("adj_eidx");
    st.adj_ts = reg<double>("adj_ts"); st.node_feat = reg<float>("node_feat"); st.edge_feat = reg<float>("edge_feat");
    st.memory = reg<float>("memory"); st.last_update = reg<float>("last_update"); st.msg_table = reg<float>("msg_table");
    st.msg_time = reg<float>("msg_time"); st.has_msg = reg<uint8_t>("has_msg"); st.params = reg<float>("params");
    st.pcache = sc.pcache ? region("pcache") : nullptr;
    st.pcache_valid = (sc.pcache == 1 || sc.pcache == 3) ? 1 : 0;
    b.roots = reg<int32_t>("roots"); b.root_ts = reg<double>("root_ts"); b.R = 90; b.K = 7;    // below the capacities, odd
    b.uniform = sc.uniform; b.seed = 1234; b.offset = 1000; b.dropout_p = sc.dropout; b.training = sc.eval ? 0 : 1;
    b.offset_dev = reg<uint64_t>("offset_dev"); b.deterministic = sc.det;
    if (sc.uniform == 1) {
      static const char* const names[PFO_MAX_LAYERS] = {"draws0", "draws1", "draws2", "draws3"};
      for (int l = 0; l < sc.L; ++l) draws[l] = reg<int64_t>(names[l]);
      b.draws = draws;
    }
    if (sc.keep) {
      static const char* const names[PFO_MAX_LAYERS] = {"keep0", "keep1", "keep2", "keep3"};
      for (int l = 0; l < sc.L; ++l) keeps[l] = reg<uint8_t>(names[l]);
      b.dropout_keep = keeps;
    }
    if (sc.n_extra) { b.extra_nodes = reg<int32_t>("extra_nodes"); b.n_extra = sc.n_extra; }
    if (sc.fused) {
      b.upd_src = reg<int32_t>("upd_src"); b.upd_dst = reg<int32_t>("upd_dst"); b.upd_ts = reg<double>("upd_ts");
      b.upd_eidx = reg<int32_t>("upd_eidx"); b.upd_B = 30;
      b.seg_in_forward = sc.fused == 2;
    }
    b.defer_join = sc.defer ? 1 : 0;
    ws = region("workspace");
  }
  int forward(hipStream_t s) { return pfo_tgn_forward(&c, &st, &b, ws, reg<float>("emb_out"), s); }
  // the caller orders stream `to` behind stream `from` with an event of its own
  void order(hipStream_t from, hipStream_t to, hipEvent_t e) { (void)hipEventRecord(e, from); (void)hipStreamWaitEvent(to, e, 0); }
};

#define CHECK(expr) do { int rc__ = (expr); if (rc__ != PFO_OK) return rc__; } while (0)

int run_scenario(const Scn& sc, hipStream_t main_s, hipStream_t other_s, hipEvent_t user_ev, hipEvent_t mid_ev, hipEvent_t top_ev) {
  K = Knobs();
  K.uses_runs = sc.uses_runs; K.runs_possible = sc.runs_possible; K.needs_winner = sc.needs_winner; K.prof = sc.prof;
  K.marks = sc.marks; K.capturing = sc.capture ? main_s : nullptr;
  Run r(sc);
  if (sc.observe) {
    const int32_t B = sc.observe == 2 ? 1 << 29 : 40;
    const int64_t N = sc.observe == 2 ? (int64_t)1 << 30 : 100, bytes = pfo_tgn_observe_workspace_bytes(&r.c, B);
    Line("scenario").i("observe_workspace_bytes", bytes);
    CHECK(pfo_tgn_observe(&r.c, &r.st, reg<int32_t>("upd_src"), reg<int32_t>("upd_dst"), reg<double>("upd_ts"),
                          reg<int32_t>("upd_eidx"), 0, B, (char*)r.ws + 64, bytes, main_s));          // (nothing to do)
    CHECK(pfo_tgn_observe(&r.c, &r.st, reg<int32_t>("upd_src"), reg<int32_t>("upd_dst"), reg<double>("upd_ts"),
                          reg<int32_t>("upd_eidx"), N, B, (char*)r.ws + 64, bytes, main_s));
    return pfo_tgn_join(main_s);
  }
  {
    // the sizes and views a caller asks for first (queries: they queue nothing)
    int64_t split = 0;
    pfo_tgn_debug d;
    memset(&d, 0, sizeof(d));
    CHECK(pfo_tgn_grad_split(&r.c, &split));
    CHECK(pfo_tgn_debug_views(&r.c, r.ws, &d));
    Line ln("scenario");
    ln.i("workspace_bytes", pfo_tgn_workspace_bytes(&r.c)).i("pcache_bytes", pfo_tgn_pcache_bytes(&r.c)).i("grad_split", split);
    FP(n_touched); FP(touched_ids); FP(h0_table); FP(slot); FP(n_core); FP(l1_ctx); FP(l1_dh1); FP(l1_dW1ovT); FP(gru_dgi);
    FP(gru_msg_rows); FI(Cp);
  }
  if (sc.pcache == 3) CHECK(pfo_tgn_refresh(&r.c, &r.st, main_s));
  if (sc.prepared) {
    CHECK(pfo_tgn_prepare(&r.c, &r.st, &r.b, r.ws, other_s));
    r.order(other_s, main_s, user_ev);
    r.b.prepared = 1;
  }
  if (sc.mid) { r.b.mid_event = mid_ev; r.b.mid_event_late = sc.mid == 2; }
  CHECK(r.forward(main_s));
  if (sc.eval) return pfo_tgn_join(main_s);
  if (!(sc.fused && sc.mem && sc.L >= 2))                      // (without memory the call returns at once)
    CHECK(pfo_tgn_update_state(&r.c, &r.st, reg<int32_t>("upd_src"), reg<int32_t>("upd_dst"), reg<double>("upd_ts"),
                               reg<int32_t>("upd_eidx"), 30, r.ws, main_s));
  if (!sc.zero_grad && !sc.top_ready && !sc.mean)
    CHECK(pfo_tgn_backward(&r.c, &r.st, &r.b, r.ws, reg<float>("d_emb"), reg<float>("grad"), main_s));
  else
    CHECK(pfo_tgn_backward_ev(&r.c, &r.st, &r.b, r.ws, reg<float>("d_emb"), reg<float>("grad"), sc.zero_grad,
                              sc.top_ready ? top_ev : nullptr, sc.mean ? reg<float>("mean_src") : nullptr, sc.mean ? 90 : 0,
                              sc.mean ? reg<float>("mean_out") : nullptr, main_s));
  float *P = reg<float>("params"), *G = reg<float>("grad"), *M1 = reg<float>("exp_avg"), *M2 = reg<float>("exp_avg_sq");
  const int64_t *lo = reg<int64_t>("adam_lo"), *hi = reg<int64_t>("adam_hi");
  const int32_t* step = reg<int32_t>("adam_step");
  if (sc.defer == 1) CHECK(pfo_tgn_adam_side(P, G, M1, M2, 1, lo, hi, step, 1e-3f, 0.9f, 0.999f, 1e-8f));
  if (sc.defer == 2) {
    CHECK(pfo_tgn_adam_side_bucket(P, G, M1, M2, 2, lo, hi, step, 1e-3f, 0.9f, 0.999f, 1e-8f, 1 | 4));
    CHECK(pfo_tgn_adam_side_bucket(P, G, M1, M2, 1, lo, hi, step, 1e-3f, 0.9f, 0.999f, 1e-8f, 2 | 4));
  }
  if (sc.defer == 4) CHECK(pfo_tgn_adam_side_bucket(P, G, M1, M2, 1, lo, hi, step, 1e-3f, 0.9f, 0.999f, 1e-8f, 0));
  if (sc.next_fwd) {
    // the next step's forward: parameters changed (an invalid cache is rebuilt), the batch is sampled afresh
    r.b.prepared = 0;
    r.b.offset += 7;
    if (r.st.pcache) r.st.pcache_valid = 0;
    hipStream_t s = sc.next_fwd == 2 ? other_s : main_s;
    CHECK(r.forward(s));
    if (s != main_s) r.order(s, main_s, user_ev);
  }
  return pfo_tgn_join(main_s);
}

// Two base scenarios - `plain` (every option off: what a bare forward / update / backward queues) and `loop` (the training
// loop's step: cached composites, state update and instance groups inside the forward, the loss mean, a deferred end and the
// bucketed optimizer step behind it) - and one factor at a time around them, plus the combinations tgn.hip itself names.
std::vector<Scn> scenarios() {
  std::vector<Scn> v;
  Scn plain; plain.name = "plain";
  Scn loop; loop.name = "loop";
  loop.pcache = 1; loop.fused = 2; loop.defer = 2; loop.next_fwd = 1; loop.mean = 1; loop.top_ready = 1; loop.mid = 2;
  loop.dropout = 0.1f; loop.marks = 1;
  v.push_back(plain);
  v.push_back(loop);
  auto add = [&](const Scn& base, const char* name, void (*change)(Scn&)) {
    Scn s = base; s.name = name; change(s); v.push_back(s);
  };
  add(plain, "plain_L1", [](Scn& s) { s.L = 1; });
  add(plain, "plain_L3", [](Scn& s) { s.L = 3; });
  add(plain, "plain_nomem", [](Scn& s) { s.mem = 0; });
  add(plain, "plain_nomem_L1", [](Scn& s) { s.mem = 0; s.L = 1; });
  add(plain, "plain_philox", [](Scn& s) { s.uniform = 2; });
  add(plain, "plain_draws", [](Scn& s) { s.uniform = 1; });
  add(plain, "plain_det", [](Scn& s) { s.det = 1; });
  add(plain, "plain_det_philox", [](Scn& s) { s.det = 1; s.uniform = 2; });
  add(plain, "plain_prof", [](Scn& s) { s.prof = 1; });
  add(plain, "plain_marks", [](Scn& s) { s.marks = 1; });
  add(plain, "plain_capture", [](Scn& s) { s.capture = 1; });
  add(plain, "plain_capture_fused", [](Scn& s) { s.capture = 1; s.fused = 2; s.pcache = 2; });
  add(plain, "plain_capture_defer", [](Scn& s) { s.capture = 1; s.defer = 3; s.mean = 1; });   // (under capture the end is never deferred)
  add(plain, "plain_small_graph", [](Scn& s) { s.n_nodes = 5000; });
  add(plain, "plain_small_graph_L1", [](Scn& s) { s.n_nodes = 5000; s.L = 1; });
  add(plain, "plain_defer_only", [](Scn& s) { s.defer = 3; });
  add(plain, "plain_pcache_valid", [](Scn& s) { s.pcache = 1; });
  add(plain, "plain_pcache_invalid", [](Scn& s) { s.pcache = 2; });
  add(plain, "plain_pcache_refresh", [](Scn& s) { s.pcache = 3; });
  add(plain, "plain_prepared", [](Scn& s) { s.prepared = 1; });
  add(plain, "plain_prepared_nomem", [](Scn& s) { s.prepared = 1; s.mem = 0; });
  add(plain, "plain_fused", [](Scn& s) { s.fused = 1; });
  add(plain, "plain_fused_seg", [](Scn& s) { s.fused = 2; });
  add(plain, "plain_fused_L1", [](Scn& s) { s.fused = 2; s.L = 1; });       // (one layer: the caller updates the state itself)
  add(plain, "plain_winner", [](Scn& s) { s.needs_winner = 1; });
  add(plain, "plain_defer_adam", [](Scn& s) { s.defer = 1; });
  add(plain, "plain_defer_adam_next_same", [](Scn& s) { s.defer = 1; s.next_fwd = 1; });
  add(plain, "plain_defer_adam_next_other", [](Scn& s) { s.defer = 1; s.next_fwd = 2; });
  add(plain, "plain_defer_bucket", [](Scn& s) { s.defer = 2; });
  add(plain, "plain_defer_bucket_next_same", [](Scn& s) { s.defer = 2; s.next_fwd = 1; });
  add(plain, "plain_defer_bucket_next_other", [](Scn& s) { s.defer = 2; s.next_fwd = 2; });
  add(plain, "plain_defer_bucket0_next_same", [](Scn& s) { s.defer = 4; s.next_fwd = 1; });
  add(plain, "plain_defer_L1", [](Scn& s) { s.defer = 1; s.L = 1; s.next_fwd = 1; });
  add(plain, "plain_defer_nomem", [](Scn& s) { s.defer = 1; s.mem = 0; s.next_fwd = 1; });
  add(plain, "plain_mid_early", [](Scn& s) { s.mid = 1; });
  add(plain, "plain_mid_late", [](Scn& s) { s.mid = 2; });
  add(plain, "plain_top_ready", [](Scn& s) { s.top_ready = 1; });
  add(plain, "plain_top_ready_L1", [](Scn& s) { s.top_ready = 1; s.L = 1; });
  add(plain, "plain_mean", [](Scn& s) { s.mean = 1; });
  add(plain, "plain_mean_prof", [](Scn& s) { s.mean = 1; s.prof = 1; });
  add(plain, "plain_mean_fused_seg", [](Scn& s) { s.mean = 1; s.fused = 2; });
  add(plain, "plain_zero_grad", [](Scn& s) { s.zero_grad = 1; });
  add(plain, "plain_extra", [](Scn& s) { s.n_extra = 12; });
  add(plain, "plain_keep", [](Scn& s) { s.keep = 1; s.dropout = 0.2f; });
  add(plain, "plain_no_runs", [](Scn& s) { s.uses_runs = 0; });
  add(plain, "plain_runs_impossible", [](Scn& s) { s.uses_runs = 0; s.runs_possible = 0; });
  add(plain, "plain_prof_L3", [](Scn& s) { s.prof = 1; s.L = 3; });
  add(plain, "observe", [](Scn& s) { s.observe = 1; });
  add(plain, "observe_pcache", [](Scn& s) { s.observe = 1; s.pcache = 1; });
  add(plain, "observe_wrap", [](Scn& s) { s.observe = 2; });
  add(plain, "plain_eval", [](Scn& s) { s.eval = 1; });
  add(plain, "plain_nomem_refresh", [](Scn& s) { s.mem = 0; s.pcache = 3; });
  add(plain, "observe_winner", [](Scn& s) { s.observe = 1; s.needs_winner = 1; });
  add(loop, "loop_L3", [](Scn& s) { s.L = 3; });
  add(loop, "loop_philox", [](Scn& s) { s.uniform = 2; });
  add(loop, "loop_det", [](Scn& s) { s.det = 1; });
  add(loop, "loop_prof", [](Scn& s) { s.prof = 1; });
  add(loop, "loop_no_marks", [](Scn& s) { s.marks = 0; });
  add(loop, "loop_capture", [](Scn& s) { s.capture = 1; s.pcache = 2; s.defer = 0; });
  add(loop, "loop_no_pcache", [](Scn& s) { s.pcache = 0; });
  add(loop, "loop_refresh", [](Scn& s) { s.pcache = 3; });
  add(loop, "loop_prepared", [](Scn& s) { s.prepared = 1; });
  add(loop, "loop_fused_only", [](Scn& s) { s.fused = 1; });
  add(loop, "loop_adam_side", [](Scn& s) { s.defer = 1; });
  add(loop, "loop_next_other", [](Scn& s) { s.next_fwd = 2; });
  add(loop, "loop_no_defer", [](Scn& s) { s.defer = 0; });
  add(loop, "loop_mid_early", [](Scn& s) { s.mid = 1; });
  add(loop, "loop_zero_grad", [](Scn& s) { s.zero_grad = 1; });
  add(loop, "loop_extra", [](Scn& s) { s.n_extra = 12; });
  add(loop, "loop_keep", [](Scn& s) { s.keep = 1; });
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s OUTDIR\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  auto open_log = [&](const std::string& name) {
    if (out) fclose(out);
    out = fopen((dir + "/" + name + ".log").c_str(), "w");
    if (!out) { fprintf(stderr, "cannot write %s/%s.log\n", dir.c_str(), name.c_str()); exit(2); }
  };
  // the library's streams and events are made once per process, at the first call that needs them: a log of its own
  open_log("setup");
  hipStream_t main_s = new_stream("main"), other_s = new_stream("other");
  hipEvent_t user_ev = new_event("caller"), mid_ev = new_event("mid_event"), top_ev = new_event("top_ready_event");
  if (!pfo_tgn_side_stream()) { fprintf(stderr, "setup: %s\n", last_error.c_str()); return 1; }
  int bad = 0;
  for (const Scn& sc : scenarios()) {
    open_log(sc.name);
    last_error.clear();
    const int rc = run_scenario(sc, main_s, other_s, user_ev, mid_ev, top_ev);
    printf("%s %d\n", sc.name, rc);
    if (rc != PFO_OK) { fprintf(stderr, "%s: %s\n", sc.name, last_error.c_str()); bad = 1; }
  }
  fclose(out);
  return bad;
}
