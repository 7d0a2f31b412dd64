// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11), the counter-based generator
// of Random123, cuRAND and torch: four 32-bit words out of a 128-bit counter and a 64-bit key, ten rounds, no state.  Plain
// C++ for the host and the device (the high half of a 32 x 32 product is __umulhi on the device, a 64-bit product on the host),
// so the attention kernels' dropout mask (egc_gat_dev.h) can be restated word for word on the CPU (tests/philox).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EGC_PHILOX_HD __host__ __device__
#else
#define EGC_PHILOX_HD
#endif

namespace egc {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // key increments (golden ratio, sqrt 3 - 1)

EGC_PHILOX_HD inline uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// out[0..3] = Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1)
EGC_PHILOX_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                        uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = philox_mulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = philox_mulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += PHILOX_W0, k1 += PHILOX_W1;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

}  // namespace egc
