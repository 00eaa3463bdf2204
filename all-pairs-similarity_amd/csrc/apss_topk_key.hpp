// apss_topk_key.hpp -- the order-preserving integer image of an fp32 score (per-query top-k, apss_topk.hpp).
// No HIP include: a CPU program can test it (tests/test_topk_key.py).
#ifndef APSS_TOPK_KEY_HPP
#define APSS_TOPK_KEY_HPP

#include <stdint.h>

#ifdef __HIPCC__
#define APSS_TOPK_HD __host__ __device__
#else
#define APSS_TOPK_HD
#endif

namespace apss {

// a < b (as floats, no NaN)  <=>  topk_key(a) < topk_key(b) (as unsigned); -0.0f and +0.0f share one key
APSS_TOPK_HD inline uint32_t topk_key(float s) {
  uint32_t b;
  __builtin_memcpy(&b, &s, sizeof(b));
  if (b == 0x80000000u) b = 0u;  // -0.0f counts as +0.0f
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the float a key came from (the canonical +0.0f for either zero)
APSS_TOPK_HD inline float topk_key_inv(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float s;
  __builtin_memcpy(&s, &b, sizeof(s));
  return s;
}

}  // namespace apss

#endif  // APSS_TOPK_KEY_HPP
