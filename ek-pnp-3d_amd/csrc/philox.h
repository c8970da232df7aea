// philox.h — the counter-based generator behind ekpnp_seed_uniform (include/ekpnp.h), shared by seed.hip (noise on the fields)
// and tracers.hip (random start positions, and the kicks of Brownian tracers: tr_kick).  Host and device run the same integer arithmetic: the same bits everywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ekpnp {

// Philox4x32-10 (Salmon et al., SC11): counter c[4], key k[2]; the key is bumped by the Weyl constants between the rounds
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the uniform number of (seed, global node, field): 53 bits of the first two output words, exact in [-1, 1)
__host__ __device__ inline double seed_uniform(uint64_t seed, uint64_t node, int field_id) {
  uint32_t c[4] = {(uint32_t)(node & 0xffffffffu), (uint32_t)(node >> 32), (uint32_t)field_id, 0u};
  philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  const uint64_t k = ((uint64_t)(c[0] >> 5) << 26) + (uint64_t)(c[1] >> 6);
  return (double)k * 0x1.0p-52 - 1.0;
}

}  // namespace ekpnp
