// Internal interface of the explanation query (explain.hip), called by pfo_tgn_explain (tgn.hip), which owns the workspace map.
#pragma once
#include "common.hpp"

// The per-slot tables of ONE forward, already addressed by the caller: level L's rows are the R roots', level L - 1's the
// R * K first-hop neighbours' (the caller skips that level's R self rows).  Every table has stride K.
struct PfoExplain {
  int32_t R, K, H, hops, m;
  const int32_t* nbr;  const float* attw;  const float* dt;  const int32_t* eidx;       // [R, K], [R, H, K], [R, K], [R, K]
  const int32_t* nbr2; const float* attw2; const float* dt2; const int32_t* eidx2;      // [R*K, K], [R*K, H, K], ..: hops == 2
  int32_t* node_out; double* weight_out; int32_t* n_valid_out; int32_t* count_out; float* age_out; int32_t* eidx_out;
  int32_t* raw_nbr;  float* raw_w;  float* raw_dt;  int32_t* raw_eidx;                  // copies of the tables above, or all NULL
  int32_t* raw_nbr2; float* raw_w2; float* raw_dt2; int32_t* raw_eidx2;
};
int pfo_explain_launch(const PfoExplain& a, hipStream_t s);
