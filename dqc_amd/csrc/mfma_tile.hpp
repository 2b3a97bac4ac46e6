// mfma_tile.hpp -- what every kernel built on 16 x 16 fp64 MFMA tiles shares: the wrapper, the fragment layout, the index of a
// triangular launch and a wave's tile transpose through LDS.
//
// f64 MFMA fragment layout (gfx950): A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
// C[row = (lane>>4) + 4*reg][col = lane&15].
#pragma once
#include "common.hpp"

namespace dqc {

typedef double v4d __attribute__((ext_vector_type(4)));

DQC_DEV v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

DQC_DEV void tri_index(long long q, int &lo, int &hi) {  // q = hi (hi + 1) / 2 + lo, lo <= hi
    long long r = (long long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > q) r--;
    while ((r + 1) * (r + 2) / 2 <= q) r++;
    hi = (int)r;
    lo = (int)(q - r * (r + 1) / 2);
}

// a wave's LDS traffic is in order; this keeps the compiler from moving its own accesses of the transpose scratch across the point
DQC_DEV void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One C tile of a wave on its way to the transposed position, through a 16 x 17 scratch of the wave's own: lane (l15 = lane & 15,
// q = lane >> 4) holds v[r] = C[row q + 4 r][col l15] and gets m[r] = C[row l15][col q + 4 r], the element (q + 4 r, l15) of C^T --
// the 16 lanes of equal q then hold 16 consecutive columns of one row of C^T.  The scratch is free again on return.
DQC_DEV void tile_transpose(double (&scratch)[16][17], const double (&v)[4], double (&m)[4]) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; r++) scratch[l15][q + 4 * r] = v[r];
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; r++) m[r] = scratch[q + 4 * r][l15];
    wave_sync();
}

}  // namespace dqc
