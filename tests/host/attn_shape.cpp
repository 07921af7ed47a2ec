// The attention's (D, H) -> (NR, H) dispatch, walked on the host: csrc/attn_shape.hpp is plain C++17 and this program
// includes nothing else of the library.
//
//   attn_shape      prints "caps <register cap> <ring cap>", then for both caps, D = 1..256 and H in {0, 1, 2, 3, 4, 8} one line
//                   "<cap> <D> <H> <returned> <calls> <NR> <H seen>" (NR and H seen are those of the last call, 0 without one)
//
// tests/test_attn_shape_cpu.py states what every line must say.
#include "attn_shape.hpp"
#include <stdio.h>

template <int CAP>
static void walk() {
  const int heads[] = {0, 1, 2, 3, 4, 8};
  for (int D = 1; D <= 256; ++D)
    for (int H : heads) {
      int calls = 0, nr_seen = 0, h_seen = 0;
      const bool ret = attn_for_shape<CAP>(D, H, [&](auto nr, auto h) {
        static_assert(decltype(nr)::value * decltype(h)::value <= CAP, "an instance beyond the cap");
        calls += 1; nr_seen = nr; h_seen = h;
      });
      printf("%d %d %d %d %d %d %d\n", CAP, D, H, ret ? 1 : 0, calls, nr_seen, h_seen);
    }
}

int main() {
  printf("caps %d %d\n", ATTN_MAX_NRH, ATTN_RING_MAX_NRH);
  walk<ATTN_MAX_NRH>();
  walk<ATTN_RING_MAX_NRH>();
  return 0;
}
