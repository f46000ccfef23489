// recip_check.hip -- checker (test infrastructure, not product code): the area reciprocal of an interior pose
// (pcore::recip_interior, pcore_fdiv.h: the compiler's division sequence for 1.0f / Y less its scaling steps, the raw
// v_rcp_f32 where Y = 0) against the compiler's IEEE `1.0f / Y`, bit for bit, on the GPU, over EVERY float inside the
// bound pcore_fdiv.h documents for an interior pose: |Y| in [2^-50, 2^29) -- 79 exponents x 2^23 mantissas -- in both
// signs, and +-0.  One thread per (sign, mantissa) walks the 79 exponents.
// Prints one JSON line {"values": N, "mismatches": M, "zero_mismatches": Z, "first_bad": "0x..."}; exit status 1 on any
// mismatch.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/bin/recip_check tools/recip_check.hip
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../perception_amd/csrc/pcore_fdiv.h"

#pragma clang fp contract(off)

constexpr uint32_t kExpLo = 127u - 50u, kExpHi = 127u + 29u;  // biased exponents [77, 156)

// out[0] mismatches in the range, out[1] mismatches at +-0, out[2] the smallest mismatching bit pattern
__global__ void check(unsigned long long* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // < 2^24: sign << 23 | mantissa
    const uint32_t sign = (i >> 23) << 31, man = i & 0x7fffffu;
    unsigned long long bad = 0ull;
    uint32_t first = 0xffffffffu;
    for (uint32_t e = kExpLo; e < kExpHi; e++) {
        const uint32_t bits = sign | (e << 23) | man;
        const float Y = __uint_as_float(bits);
        const float want = 1.0f / Y;
        const float got = pcore::recip_interior(Y);
        if (__float_as_uint(want) != __float_as_uint(got)) {
            bad++;
            first = min(first, bits);
        }
    }
    if (bad) {
        atomicAdd(&out[0], bad);
        atomicMin(&out[2], (unsigned long long)first);
    }
    if (man == 0u) {  // two threads: +0 and -0
        const float Z = __uint_as_float(sign);
        if (__float_as_uint(1.0f / Z) != __float_as_uint(pcore::recip_interior(Z))) atomicAdd(&out[1], 1ull);
    }
}

int main() {
    unsigned long long *d, h[3] = {0, 0, ~0ull};
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
    if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) return 2;
    const int threads = 256, blocks = (1 << 24) / threads;
    hipLaunchKernelGGL(check, dim3(blocks), dim3(threads), 0, 0, d);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("{\"values\": %.0f, \"mismatches\": %llu, \"zero_mismatches\": %llu, \"first_bad\": \"0x%08llx\"}\n",
           (double)(kExpHi - kExpLo) * (double)(1 << 24) + 2.0, h[0], h[1], h[0] ? h[2] : 0ull);
    return h[0] == 0 && h[1] == 0 ? 0 : 1;
}
