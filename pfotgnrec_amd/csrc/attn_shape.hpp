// The shapes the attention kernels are instantiated for, and the one switch from a run-time (D, H) to an instance.  Plain
// C++17, no HIP: tests/host/attn_shape.cpp walks it on the host.  A kernel is a template over NR = ceil(D / 64) column groups
// of 64 lanes (1..4) and H heads (1, 2, 4); a family is instantiated for the pairs with NR H <= its cap and for no other.
#pragma once
#include <type_traits>

constexpr int ATTN_MAX_NRH = 16;        // the register forms: every pair
constexpr int ATTN_RING_MAX_NRH = 12;   // the key-ring forms and the run-merged backward: all but (4, 4), which takes a register form

template <int MAX_NRH, int NR, typename F>
inline bool attn_for_heads(int H, F& f) {
  auto go = [&](auto h) {
    if constexpr (NR * decltype(h)::value <= MAX_NRH) { f(std::integral_constant<int, NR>{}, h); return true; }
    else return false;
  };
  switch (H) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 4: return go(std::integral_constant<int, 4>{});
  }
  return false;
}
// f(integral_constant<NR>, integral_constant<H>) for the pair (D, H) names, once; false, and no call, for any other pair
template <int MAX_NRH, typename F>
inline bool attn_for_shape(int D, int H, F&& f) {
  switch (D > 0 ? (D + 63) / 64 : 0) {
    case 1: return attn_for_heads<MAX_NRH, 1>(H, f);
    case 2: return attn_for_heads<MAX_NRH, 2>(H, f);
    case 3: return attn_for_heads<MAX_NRH, 3>(H, f);
    case 4: return attn_for_heads<MAX_NRH, 4>(H, f);
  }
  return false;
}
