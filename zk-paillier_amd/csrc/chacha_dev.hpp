// chacha_dev.hpp — the ChaCha20 block function of RFC 8439 (20 rounds, 32-bit block counter in state word 12) for one lane:
// the 16 state words live in VGPRs, the rounds are add / xor / rotate only (no LDS, no cross-lane traffic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zkp {

#define ZKP_CHACHA_QR(a, b, c, d)                         \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 16);      \
  c += d; b ^= c; b = __builtin_rotateleft32(b, 12);      \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 8);       \
  c += d; b ^= c; b = __builtin_rotateleft32(b, 7);

// out[j] = keystream word j of the block (key, counter, nonce words n0 n1 n2), in RFC order
__device__ __forceinline__ void chacha20_block(const uint32_t (&key)[8], uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t (&out)[16]) {
  const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                           key[4], key[5], key[6], key[7], counter, n0, n1, n2};
  uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7];
  uint32_t x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
#pragma unroll 1
  for (int round = 0; round < 10; round++) {
    ZKP_CHACHA_QR(x0, x4, x8, x12) ZKP_CHACHA_QR(x1, x5, x9, x13) ZKP_CHACHA_QR(x2, x6, x10, x14) ZKP_CHACHA_QR(x3, x7, x11, x15)
    ZKP_CHACHA_QR(x0, x5, x10, x15) ZKP_CHACHA_QR(x1, x6, x11, x12) ZKP_CHACHA_QR(x2, x7, x8, x13) ZKP_CHACHA_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + in[0]; out[1] = x1 + in[1]; out[2] = x2 + in[2]; out[3] = x3 + in[3];
  out[4] = x4 + in[4]; out[5] = x5 + in[5]; out[6] = x6 + in[6]; out[7] = x7 + in[7];
  out[8] = x8 + in[8]; out[9] = x9 + in[9]; out[10] = x10 + in[10]; out[11] = x11 + in[11];
  out[12] = x12 + in[12]; out[13] = x13 + in[13]; out[14] = x14 + in[14]; out[15] = x15 + in[15];
}
#undef ZKP_CHACHA_QR

}  // namespace zkp
