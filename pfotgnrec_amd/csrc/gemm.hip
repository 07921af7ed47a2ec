// The contraction's dispatcher: host code only.  It decides which kernel runs (gemm_plan, tn_group_plan), fills the argument
// blocks and brackets the launches with the profiler; it defines no kernel and launches none itself.  The kernels live one
// family per file - gemm_f32.hip (exact fp32 tile), gemm_bx.hip (image kernels), gemm_tn_bx.hip (grouped weight gradients and
// the slab fold) - and are started through the launch functions of gemm_dev.hpp.
#include "gemm_dev.hpp"
#include <algorithm>
#include <string.h>

// launch thresholds of the dispatch (pfo_gemm_launch, pfo_gemm_tn_group_launch)
constexpr int F32_BIG_MIN_TILES = 400;   // row-major launches of the fp32 kernel: fewer 128 x 176 tiles take its 32-row tile (a threshold of its own)
constexpr int BX_MIN_TILES = 400;   // row-major launches with images: fewer 128 x 176 tiles take the 32-row kernel, more the 128-row ones
constexpr int BX_AREG8_MIN = 512;   // ... the 128-row form as eight single-strip wavefronts (gemm_bx_areg8_kernel) from this many tiles on
constexpr int TN8_MIN_ROWS = 500;   // weight-gradient launches whose problems all have >= this many rows take 256-row tiles

// ---------------------------------------------------------------------------------------------
// The dispatch.  What a launcher decides before it touches the device is one plain record, filled by a pure function of the
// descriptor: pointers are tested for null and alignment and never followed, no HIP call is made.  The launcher switches on
// the record and the pfo_*_plan queries (gemm.hpp) return it, so the tests' statement of the rule is held to the rule that runs.
struct GemmPlan {
  int form = -1;                 // PFO_GEMM_FORM_*
  bool vec = false;              // float4 operand loads (the fp32 kernels' template flag)
  dim3 grid;
  int block = GEMM_THREADS;
  int kind = -1;                 // PFO_PROF_* of the contraction kernel
  int nsplit = 1, chunk = 0;     // split-K
  int xcd_tm = 0, xcd_tn = 0;    // pfo_gemm_launch: GemmDev's tile order
  int b_img_rows = 0;            // pfo_gemm_launch: > 0 = an image kernel reads b_img / b_img2
  int xcd_map = 0, tiles = 0;    // the grouped launch: TnGroupDev's grid order, tiles of one split ...
  int64_t per_split = 0;         // ... and floats of one split's slabs
  struct { int tile_begin, tn; int64_t slab_off; } prob[TN_MAX_PROBLEMS];
};
// a refusal names the launcher the plan belongs to (`who`), as it did when the checks stood in the launcher's body
#define PLAN_REQUIRE(cond, msg)                                                                  \
  do { if (!(cond)) { pfo_set_error("%s: %s", who, msg); return PFO_ERR_INVALID; } } while (0)

// K in nsplit chunks of whole k-tiles: at most `want` of them and none that four k-tiles would not fill
static void split_k(int K, int64_t want, int& nsplit, int& chunk) {
  nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(want, pfo_ceil_div(K, 4 * BK)));
  chunk = (int)pfo_align_up(pfo_ceil_div(K, nsplit), BK);
  nsplit = (int)pfo_ceil_div(K, chunk);
}

// float4 loads of the A operands / of the B operands of every source in use
static void gemm_vec_ok(const PfoGemm& g, bool& a_vec, bool& b_vec) {
  a_vec = b_vec = true;
  for (int s = 0; s < 2; ++s) {
    if (s == 1 && g.K[1] == 0) continue;
    a_vec = a_vec && aligned4(g.A[s]) && (g.lda[s] % 4) == 0 && (g.a_bs[s] % 4) == 0 &&
            (g.a_kmajor ? (g.M % 4) == 0 : (g.K[s] % 4) == 0);
    b_vec = b_vec && aligned4(g.B[s]) && (g.ldb[s] % 4) == 0 && (g.b_bs[s] % 4) == 0 &&
            (g.b_kmajor ? (g.N % 4) == 0 : (g.K[s] % 4) == 0);
  }
}

static int gemm_plan(const PfoGemm& g, GemmPlan& p) {
  const char* const who = "pfo_gemm_launch";
  PLAN_REQUIRE(g.M > 0 && g.N > 0 && g.K[0] > 0 && g.batch >= 1, "bad sizes");
  PLAN_REQUIRE(g.A[0] && g.B[0] && g.C, "null operand");
  PLAN_REQUIRE(g.K[1] == 0 || (g.A[1] && g.B[1]), "null operand (source 2)");
  bool a_vec, b_vec;
  gemm_vec_ok(g, a_vec, b_vec);
  p.vec = a_vec && b_vec;
  // the launch takes an image kernel (gemm_bx.hip) exactly when this holds; what those kernels, or the fp32 one, would not read
  // is refused, not dropped
  const bool img_launch = !g.a_kmajor && g.b_img && (g.K[1] == 0 || g.b_img2) && a_vec && g.batch == 1;
  // b_idx gathers the k rows of a k-major B in the fp32 kernel; a weight image is built from the ungathered operand
  PLAN_REQUIRE(!g.b_idx || (g.b_kmajor && !img_launch), "b_idx needs a k-major B and a launch that takes no weight image");
  PLAN_REQUIRE(!g.a_kmajor || (!g.a_idx[0] && !g.a_idx[1]), "a_idx needs a row-major A");
  // the row-gathered addend exists in the epilogue of the image kernels only
  PLAN_REQUIRE(!g.add_src || img_launch, "add_src needs a weight-image launch (row-major 16-byte aligned A, b_img, batch 1)");
  p.kind = g.m_dev ? PFO_PROF_GEMM_DEVM : (g.a_kmajor ? PFO_PROF_GEMM_TN : (g.b_kmajor ? PFO_PROF_GEMM_NN : PFO_PROF_GEMM_NT));
  const int tm = (int)pfo_ceil_div(g.M, BM), tn = (int)pfo_ceil_div(g.N, BN);
  if (g.a_kmajor) {
    PLAN_REQUIRE(g.K[1] == 0, "k-major A supports one source");
    // weight gradient: few output tiles, long K -> split K over workgroups, deterministic slab reduce
    int nsplit, chunk;
    split_k(g.K[0], (int)pfo_ceil_div(512, (int64_t)tm * tn * g.batch), nsplit, chunk);
    if (nsplit > 1 && g.b_kmajor && g.slabs) {
      // the weight-gradient form goes through the grouped split-K launch (one problem), which plans its own grid and split
      PLAN_REQUIRE(g.batch == 1, "split-K with batch is not supported");
      PLAN_REQUIRE(!g.bias && !g.relu && !g.row_zero && !g.relu_src, "split-K takes no epilogue");
      p.form = PFO_GEMM_FORM_TN_GROUP; p.nsplit = nsplit; p.chunk = chunk; p.grid = dim3(0, 0, 0); p.block = 0; p.kind = -1;
      return PFO_OK;
    }
    p.form = PFO_GEMM_FORM_F32_128; p.grid = dim3(tm, tn, g.batch);
    return PFO_OK;
  }
  const int64_t big_tiles = (int64_t)tm * tn * g.batch;
  if (!img_launch) {
    // the caller fused two sources whose float B operands may differ in layout: only the image kernels can take that
    if (g.K[1] > 0 && g.b_img2) {
      pfo_set_error("%s: a two-source launch with weight images needs 16-byte aligned row-major A operands", who);
      return PFO_ERR_INVALID;
    }
    // tile rows per workgroup: 128, or 32 for launches where 128-row tiles would leave most of the 256 CUs without work
    const bool small = big_tiles < F32_BIG_MIN_TILES;
    p.form = small ? PFO_GEMM_FORM_F32_32 : PFO_GEMM_FORM_F32_128;
    p.grid = dim3((unsigned)pfo_ceil_div(g.M, small ? 32 : BM), tn, g.batch);
    return PFO_OK;
  }
  // the split contraction on the caller's pre-split image of B (pfo_bimg_launch): 32-row workgroups for launches of fewer
  // than BX_MIN_TILES 128-row tiles, the 128-row kernels from there on (gemm_bx.hip; bx_force: tests pick one)
  p.b_img_rows = (int)pfo_align_up(g.N, BN);
  if (g.bx_force == 2 || (!g.bx_force && big_tiles < BX_MIN_TILES)) {
    p.kind = PFO_PROF_GEMM_BX_SKINNY;
    // few row tiles (< one per CU even with 176-column workgroups): 64-column workgroups fill the chip three times better
    const int64_t rows = pfo_ceil_div(g.M, SK_ROWS);
    const bool narrow = rows * tn < 512;
    p.form = narrow ? PFO_GEMM_FORM_SKINNY4 : PFO_GEMM_FORM_SKINNY11;
    p.grid = dim3((unsigned)rows, narrow ? (unsigned)pfo_ceil_div(g.N, 64) : tn, 1);
    return PFO_OK;
  }
  p.kind = PFO_PROF_GEMM_BX;
  p.grid = dim3((unsigned)tm, tn, 1);
  if (tn > 1) { p.xcd_tm = tm; p.xcd_tn = tn; p.grid = dim3((unsigned)(pfo_ceil_div(tm, 8) * 8 * tn), 1, 1); }
  // short contraction, many columns, plain stores: the A-stationary form (gemm_bx_astat_kernel)
  const bool astat = g.K[1] == 0 && g.K[0] <= AS_TMAX * BK && (g.N % 32) == 0 && g.N >= 352 && g.N <= AS_NMAX && (g.ldc % 4) == 0 &&
                     aligned4(g.C) && !g.bias && !g.relu && !g.relu_src && !g.add_src && !g.accumulate && !g.row_scale && !g.row_zero &&
                     g.M >= 128 * 256;
  // (eight single-strip wavefronts from BX_AREG8_MIN workgroups on; below one workgroup per slot the four-wavefront form's
  //  fewer barriers win - QX / GRU shapes at 470 workgroups: 32.0 against 35.7 us)
  if (astat) { p.form = PFO_GEMM_FORM_ASTAT; p.grid = dim3((unsigned)pfo_ceil_div(g.M, 128)); }
  else if (big_tiles >= BX_AREG8_MIN) { p.form = PFO_GEMM_FORM_AREG8; p.block = 512; }
  else p.form = PFO_GEMM_FORM_AREG;
  return PFO_OK;
}

static int tn_group_plan(const PfoTnProblem* probs, int n, int K, int64_t slab_floats, GemmPlan& p) {
  const char* const who = "pfo_gemm_tn_group_launch";
  PLAN_REQUIRE(n >= 1 && n <= TN_MAX_PROBLEMS && K > 0 && probs, "bad arguments");
  // flattened tile starts with 128-row tiles [0] and with 256-row tiles of eight wavefronts [1] (one workgroup per CU): the
  // latter when every problem admits float4 loads and is at least TN8_MIN_ROWS tall
  int begin[2][TN_MAX_PROBLEMS], tiles[2] = {0, 0};
  bool vec = true, tall = true;
  for (int i = 0; i < n; ++i) {
    const PfoTnProblem& s = probs[i];
    PLAN_REQUIRE(s.A && s.B && s.C && s.M > 0 && s.N > 0, "bad problem");
    vec = vec && aligned4(s.A) && aligned4(s.B) && (s.lda % 4) == 0 && (s.ldb % 4) == 0 && (s.M % 4) == 0 && (s.N % 4) == 0;
    tall = tall && s.M >= TN8_MIN_ROWS;
    const int N = s.N + (s.bias_out ? 1 : 0);     // the bias gradient is carried as column N
    p.prob[i].tn = (int)pfo_ceil_div(N, BN);
    for (int h = 0; h < 2; ++h) { begin[h][i] = tiles[h]; tiles[h] += (int)pfo_ceil_div(s.M, BM << h) * p.prob[i].tn; }
    p.prob[i].slab_off = p.per_split;             // scaled by nsplit below
    p.per_split += (int64_t)s.M * N;
  }
  const int tn8 = vec && tall;
  p.vec = vec;
  p.tiles = tiles[tn8];
  // one full round of resident workgroups, never a nearly empty second one: 2 per CU x 256 CUs in the 128-row form (768 = 3 per
  // CU also fits: LDS 3 x 49.6 KB, 3 x 120 registers)
  split_k(K, (tn8 ? 256 : 512) / std::max(1, p.tiles), p.nsplit, p.chunk);
  PLAN_REQUIRE(slab_floats >= p.per_split * p.nsplit, "split-K workspace too small");
  for (int i = 0; i < n; ++i) { p.prob[i].tile_begin = begin[tn8][i]; p.prob[i].slab_off *= p.nsplit; }
  p.form = !vec ? PFO_GEMM_FORM_TN_F32 : (tn8 ? PFO_GEMM_FORM_TN_BX8 : PFO_GEMM_FORM_TN_BX);
  p.kind = !vec ? PFO_PROF_GEMM_TN : (tn8 ? PFO_PROF_GEMM_TN_BX8 : PFO_PROF_GEMM_TN_BX);
  p.block = tn8 ? 512 : GEMM_THREADS;
  p.xcd_map = vec && p.nsplit > 1;
  p.grid = p.xcd_map ? dim3(p.tiles * p.nsplit, 1) : dim3(p.tiles, p.nsplit);
  return PFO_OK;
}

// the queries: the plan as int32 out[PFO_GEMM_PLAN_INTS] (include/pfotgn.h); the form, or -1 with the launcher's message
static int plan_out(const GemmPlan& p, int32_t* out) {
  const int32_t v[PFO_GEMM_PLAN_INTS] = {p.form, p.vec, (int32_t)p.grid.x, (int32_t)p.grid.y, (int32_t)p.grid.z, p.block, p.nsplit, p.chunk, p.kind};
  memcpy(out, v, sizeof(v));
  return p.form;
}
int pfo_gemm_plan(const PfoGemm& g, int32_t* out) {
  GemmPlan p;
  return gemm_plan(g, p) == PFO_OK ? plan_out(p, out) : -1;
}
int pfo_gemm_tn_group_plan(const PfoTnProblem* probs, int n, int K, int64_t slab_floats, int32_t* out) {
  GemmPlan p;
  return tn_group_plan(probs, n, K, slab_floats, p) == PFO_OK ? plan_out(p, out) : -1;
}

int pfo_gemm_tn_group_launch(const PfoTnProblem* probs, int n, int K, const int32_t* k_dev, float* slabs,
                             int64_t slab_floats, hipStream_t stream) {
  PFO_REQUIRE(slabs, "bad arguments");
  GemmPlan p;
  if (int rc = tn_group_plan(probs, n, K, slab_floats, p)) return rc;
  TnGroupDev g;
  memset(&g, 0, sizeof(g));
  double flops = 0;
  for (int i = 0; i < n; ++i) {
    const PfoTnProblem& s = probs[i];
    TnProbDev& d = g.p[i];
    d.A = s.A; d.lda = s.lda; d.B = s.B; d.ldb = s.ldb; d.b_idx = s.b_idx;
    d.C = s.C; d.ldc = s.ldc;
    d.bias_out = s.bias_out; d.bias_accumulate = s.bias_accumulate; d.c_accumulate = s.c_accumulate;
    d.M = s.M; d.N_real = s.N; d.N = s.N + (s.bias_out ? 1 : 0);
    d.tn = p.prob[i].tn; d.tile_begin = p.prob[i].tile_begin; d.slab_off = p.prob[i].slab_off;
    flops += 2.0 * s.M * s.N * (double)K;
  }
  g.n = n; g.K = K; g.nsplit = p.nsplit; g.chunk = p.chunk; g.total_tiles = p.tiles; g.k_dev = k_dev; g.slabs = slabs;
  g.xcd_map = p.xcd_map;
  const bool bx = p.form != PFO_GEMM_FORM_TN_F32;
  pfo_prof_begin(stream);
  if (int rc = bx ? gemm_tn_group_bx_run(p.form, p.grid, dim3(p.block), g, stream) : gemm_tn_group_f32_run(p.grid, dim3(p.block), g, stream))
    return rc;
  // the GEMM kernel alone; with a device-side K bound the work is (flops per k-row) x the count read back at collect time
  if (bx) pfo_prof_end_dev(p.kind, flops / (double)K, k_dev, K, stream);
  if (bx) pfo_prof_begin(stream);                               // the slab fold is a family of its own: slabs in, matrices out
  if (int rc = tn_group_reduce_run(dim3((unsigned)std::min<int64_t>(1024, pfo_ceil_div(p.per_split, 256))), g, stream)) return rc;
  if (!bx) pfo_prof_end_dev(p.kind, flops / (double)K, k_dev, K, stream);
  else pfo_prof_end(PFO_PROF_TN_REDUCE, (double)p.per_split * (p.nsplit + 1) * sizeof(float), stream);
  return PFO_OK;
}

static void to_dev(const PfoGemm& g, GemmDev& d) {
  d.xcd_tm = d.xcd_tn = 0;
  for (int s = 0; s < 2; ++s) {
    d.A[s] = g.A[s]; d.lda[s] = g.lda[s]; d.a_idx[s] = g.a_idx[s];
    d.B[s] = g.B[s]; d.ldb[s] = g.ldb[s]; d.K[s] = g.K[s];
    d.a_bs[s] = g.a_bs[s]; d.b_bs[s] = g.b_bs[s];
  }
  d.b_idx = g.b_idx;
  d.C = g.C; d.ldc = g.ldc; d.bias = g.bias; d.row_scale = g.row_scale; d.rs_ld = g.rs_ld; d.row_zero = g.row_zero;
  d.relu_src = g.relu_src; d.relu_ld = g.relu_ld; d.M = g.M; d.N = g.N; d.m_dev = g.m_dev;
  d.add_src = g.add_src; d.add_ld = g.add_ld; d.add_idx = g.add_idx;
  d.relu = g.relu; d.accumulate = g.accumulate; d.nsplit = 1; d.split_chunk = 0;
  d.c_bs = g.c_bs; d.bias_bs = g.bias_bs; d.rs_bs = g.rs_bs;
  d.n_real = g.N; d.slab_base = g.slabs; d.dyn_chunk = 0;
  d.b_img = nullptr; d.b_img_rows = 0; d.b_img2 = nullptr;
}

int pfo_gemm_launch(const PfoGemm& g, hipStream_t stream) {
  GemmPlan p;
  if (int rc = gemm_plan(g, p)) return rc;
  if (p.form == PFO_GEMM_FORM_TN_GROUP) {
    PfoTnProblem q;
    q.A = g.A[0]; q.lda = g.lda[0]; q.B = g.B[0]; q.ldb = g.ldb[0]; q.b_idx = g.b_idx; q.M = g.M; q.N = g.N;
    q.C = g.C; q.ldc = g.ldc; q.c_accumulate = g.accumulate;
    return pfo_gemm_tn_group_launch(&q, 1, g.K[0], g.m_dev, g.slabs, g.slab_floats, stream);
  }
  GemmDev d;
  to_dev(g, d);
  d.xcd_tm = p.xcd_tm; d.xcd_tn = p.xcd_tn;
  if (p.b_img_rows) { d.b_img = g.b_img; d.b_img_rows = p.b_img_rows; d.b_img2 = g.b_img2; }
  const dim3 block(p.block);
  pfo_prof_begin(stream);
  const bool f32 = p.form == PFO_GEMM_FORM_F32_128 || p.form == PFO_GEMM_FORM_F32_32;
  if (int rc = f32 ? gemm_f32_run(p.form, p.vec, g.a_kmajor != 0, g.b_kmajor != 0, p.grid, block, d, stream)
                   : gemm_bx_run(p.form, p.grid, block, d, stream))
    return rc;
  // a device-side extent (rows, or the K of a k-major A) scales the work: read back when the records are collected
  const double flops = 2.0 * g.M * g.N * ((double)g.K[0] + g.K[1]) * g.batch;
  if (g.m_dev) pfo_prof_end_dev(p.kind, flops / (double)(g.a_kmajor ? g.K[0] : g.M), g.m_dev, g.a_kmajor ? g.K[0] : g.M, stream);
  else pfo_prof_end(p.kind, flops, stream);
  return PFO_OK;
}

int pfo_gemm_multi_launch(const PfoGemm* list, int n, hipStream_t stream) {
  PFO_REQUIRE(list && n >= 1, "bad arguments");
  for (int base = 0; base < n; base += MULTI_MAX) {
    const int cnt = std::min(MULTI_MAX, n - base);
    MultiDev g;
    memset(&g, 0, sizeof(g));
    bool vec = true;
    int tiles = 0;
    for (int i = 0; i < cnt; ++i) {
      const PfoGemm& s = list[base + i];
      PFO_REQUIRE(s.M > 0 && s.N > 0 && s.K[0] > 0 && s.A[0] && s.B[0] && s.C, "bad problem");
      PFO_REQUIRE(!s.m_dev && !s.slabs && !s.add_src, "multi launch takes plain problems only");
      PFO_REQUIRE((!s.b_idx || s.b_kmajor) && (!s.a_kmajor || (!s.a_idx[0] && !s.a_idx[1])), "a gather the problem's layout does not read");
      to_dev(s, g.p[i]);
      g.layout[i] = (s.a_kmajor ? 2 : 0) + (s.b_kmajor ? 1 : 0);
      g.tm[i] = (int)pfo_ceil_div(s.M, 32);
      g.tn[i] = (int)pfo_ceil_div(s.N, 64);            // gemm_tile's TINY shape: 32 x 64
      g.tile_begin[i] = tiles;
      tiles += g.tm[i] * g.tn[i] * s.batch;
      bool a_vec, b_vec;
      gemm_vec_ok(s, a_vec, b_vec);
      vec = vec && a_vec && b_vec;
    }
    g.n = cnt;
    double mflops = 0;
    for (int i = 0; i < cnt; ++i) mflops += 2.0 * list[base + i].M * list[base + i].N * (double)list[base + i].K[0] * list[base + i].batch;
    pfo_prof_begin(stream);
    if (int rc = gemm_multi_run(vec, dim3(tiles), g, stream)) return rc;
    pfo_prof_end(PFO_PROF_GEMM_MULTI, mflops, stream);
  }
  return PFO_OK;
}


// ---------------------------------------------------------------------------------------------
extern "C" int pfo_gemm_f32(const float* A, int64_t lda, int32_t a_kmajor, const float* B, int64_t ldb,
                            int32_t b_kmajor, float* C, int64_t ldc, const float* bias, int32_t M, int32_t N, int32_t K,
                            int32_t relu, float* workspace, int64_t workspace_floats, void* stream) {
  PfoGemm g;
  g.A[0] = A; g.lda[0] = lda; g.B[0] = B; g.ldb[0] = ldb; g.K[0] = K;
  g.C = C; g.ldc = ldc; g.bias = bias; g.M = M; g.N = N; g.relu = relu;
  g.a_kmajor = a_kmajor; g.b_kmajor = b_kmajor;
  g.slabs = workspace; g.slab_floats = workspace_floats;
  if (a_kmajor && bias) { pfo_set_error("pfo_gemm_f32: k-major A takes no bias"); return PFO_ERR_INVALID; }
  return pfo_gemm_launch(g, (hipStream_t)stream);
}

// "bf16x3" in these two ABI names is historical: the first split format had three bf16 pieces per element.  The only format
// now is two fp16 pieces and three products per block (gemm_dev.hpp); the names stay because the ABI does.
extern "C" int64_t pfo_gemm_bf16x3_workspace_bytes(int32_t N, int32_t K) { return pfo_bimg_bytes(N, K); }

extern "C" int pfo_gemm_bf16x3(const float* A, int64_t lda, const float* B, int64_t ldb, int32_t b_kmajor, float* C,
                               int64_t ldc, const float* bias, int32_t M, int32_t N, int32_t K, int32_t relu,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  PFO_REQUIRE(A && B && C && workspace, "null operand");
  PFO_REQUIRE(M > 0 && N > 0 && K > 0, "bad sizes");
  PFO_REQUIRE(workspace_bytes >= pfo_bimg_bytes(N, K), "workspace too small for the image of B");
  PFO_REQUIRE(aligned4(A) && (lda % 4) == 0 && (K % 4) == 0, "A must be 16-byte aligned with lda and K multiples of 4");
  PfoBimg im;
  im.src = B; im.ld = ldb; im.N = N; im.K = K; im.trans = b_kmajor ? 1 : 0; im.dst = workspace;
  if (int rc = pfo_bimg_launch(&im, 1, (hipStream_t)stream)) return rc;
  PfoGemm g;
  g.A[0] = A; g.lda[0] = lda; g.B[0] = B; g.ldb[0] = ldb; g.K[0] = K; g.C = C; g.ldc = ldc; g.bias = bias;
  g.M = M; g.N = N; g.relu = relu; g.b_kmajor = b_kmajor ? 1 : 0; g.b_img = workspace;
  g.bx_force = M <= 4096 ? 2 : 1;            // short operands take the 32-row kernel, as in the TGN step
  return pfo_gemm_launch(g, (hipStream_t)stream);
}
