// Host check of egc_amd/csrc/egc_philox.h: reads lines "c0 c1 c2 c3 k0 k1" (hexadecimal) from stdin and prints the four words of
// Philox4x32-10 for each, hexadecimal, one line per input line.  Host code only, nothing linked from the project.
#include <cinttypes>
#include <cstdio>

#include "egc_philox.h"

int main() {
  uint32_t v[6];
  while (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
    uint32_t w[4];
    egc::philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5], w);
    std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", w[0], w[1], w[2], w[3]);
  }
  return 0;
}
