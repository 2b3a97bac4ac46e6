// grid_vxc.hip -- the Vxc matrix V = (M + M^T) / 2, M = Phi^T Psi, from the cached AO matrix on the grid
// (reference: HamiltonCGTO._get_vxc_from_potinfo, hcgto.py:445-495, which runs it as chunked torch.matmul + einsum on the
// CPU).  The density pass over the same AO matrix lives in grid_density.hip.
//
//   Psi = w (vrho Phi + sum_d 2 vgrad_d dPhi_d)      GGA: four AO components (dqc_grid_vxc, dqc_grid_vxc_raw)
//   Psi = w v Phi_b                                  one component; Phi_b == Phi: LDA Vxc, the tau terms of a meta-GGA
//                                                    (symmetric M), Phi_b != Phi: the "pair" form (dqc_grid_vxc_pair)
//
// Every kernel here is an fp64 MFMA (v_mfma_f64_16x16x4_f64) GEMM, split-K over slabs of grid points, whose operands stream
// from HBM once per block: 16-point chunks of (Phi, Psi) are staged in double-buffered LDS -- Psi is formed on the way in, so
// nothing of size (ngrid, nao) is ever written back -- by PRODUCER waves while CONSUMER waves do nothing but fragment reads
// and MFMAs; the blocks' partial sums meet in fp64 atomics (deterministic mode: fixed point) and symmetrize_kernel closes.
// Four kernel families, chosen by the number T of 16 x 16 tile rows and the form (grid_vxc_impl at the end of the file):
//   vxc_ws_kernel    T <= 9 (GGA), T <= 13 (pair), T <= 9 and T = 14, 15 (one operand): linear tile split over 1-2 blocks per slab
//   vxc_wsu_kernel   10 <= T <= 13, one operand, no gradient term:       one block per slab, upper-triangular tiles
//   vxc_wsd_kernel   10 <= T <= 13, GGA:                                 the same, two MFMAs per off-diagonal tile
//   vxc_ws2_kernel   everything larger:                                  rectangles of <= 9 x 12 tiles per block
//
// Shared by all of them:
//   ld  = 16 T: rows / columns of the output matrix and the tile-padded width of an AO row that is staged;
//   lda = row stride of the AO arrays in HBM (dqc_ao_stride).  Where lda < ld, columns lda .. ld - 1 of a staged row are the
//         first doubles of the next row: finite values that only reach rows / columns of M that symmetrize_kernel zeroes;
//   LS  = LDS row stride of a staged chunk, == 16 (mod 32) so that the ds_read_b64 fragment reads are conflict-free.
//
// f64 MFMA fragment layout (gfx950): A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
// C[row = (lane>>4) + 4*reg][col = lane&15].
#include <utility>

#include "grid_common.hpp"

namespace dqc {

int vxc_cus_cap();  // host.hip: dqc_set_vxc_cus / DQC_VXC_CUS

// fixed-point scale of the split-K accumulation into V in deterministic mode (0: fp64 atomics); common.hpp: acc_add
__device__ double g_vxc_det_scale = 0.0;

constexpr int VXC_WAVES = 8;    // consumer (MFMA) waves per block

// ---------------------------------------------------------------------------------------------
// Vxc, wave-specialised, linear tile split (small bases).  Measured on MI355X: a SIMD reaches the fp64 MFMA peak (one
// 16x16x4 per 64.6 cycles, 78 TF chip-wide) only while TWO of its waves are issuing MFMAs; a single issuing wave
// gets one per 140 cycles (36 TF).  A kernel whose waves all alternate MFMA work with loads, the Psi combination and LDS
// writes leaves fewer than two waves per SIMD feeding the matrix pipe for part of every chunk.  Here a block is
// 16 waves: waves 0-7 (two per SIMD) are CONSUMERS that do nothing but fragment reads + MFMAs; waves 8-15 (two per
// SIMD) are PRODUCERS that fetch the next chunk's four AO components (buffer loads: no VALU address arithmetic), form
// Psi and write the (Phi, Psi) chunk to the other LDS buffer.  An fp64 MFMA occupies the SIMD's vector ALU, so the
// producers' VALU work cannot overlap the MFMAs: it runs in a window between two s_barriers per chunk during which the
// consumers wait; the loads fly during the MFMA phase (see the comments in the kernel and DESIGN.md, section 3).
//
// Work split: the grid points are cut into slabs (split-K); the T x T output tiles (sym: the upper triangle) are cut into
// `nsplit` runs of `tiles_per_split` consecutive tiles, one block per (slab, run), and a run is dealt evenly to the block's 8
// consumer waves (ws_deal).  XCD-aware block decode: blocks are dispatched round-robin over the 8 XCDs, so the nsplit blocks
// that share a slab get ids 8 apart -- same XCD, dispatched together, and the slab is fetched from HBM once.  Epilogue: every
// wave adds its accumulator tiles to M with fp64 atomics (acc_add; fixed point in deterministic mode).
// ---------------------------------------------------------------------------------------------
#ifndef VWS_PROD_THREADS
#define VWS_PROD_THREADS 512
#endif
constexpr int VWS_PROD = VWS_PROD_THREADS;    // producer threads (8 waves: two per SIMD)
constexpr int VWS_NT = 512 + VWS_PROD;        // threads per block
constexpr int VWS2_PROD = 256, VWS2_NT = 512 + VWS2_PROD;  // vxc_ws2_kernel: 4 producer waves

#ifdef VXC_TRACE  // per-chunk timeline of vxc_ws_kernel for tools/ubench/vxc_trace.hip (100 MHz ticks)
constexpr int VXC_TRACE_MAXC = 192;
__device__ long long g_vxc_trace[256 * 2 * (VXC_TRACE_MAXC + 2)];
#define VXC_TRACE_POINT(role, slot) \
    if (lane == 0 && blockIdx.x < 256 && (slot) < VXC_TRACE_MAXC + 2) g_vxc_trace[(blockIdx.x * 2 + (role)) * (VXC_TRACE_MAXC + 2) + (slot)] = wall_clock64()
#else
#define VXC_TRACE_POINT(role, slot)
#endif

// LDS layout of a (Phi, Psi) chunk in vxc_ws_kernel:  element (buffer b, component X, point k, column j) sits at
//     b * VWS_BUF + X * VWS_XS + (k >> 2) * VWS_GS + (k & 3) * ld + j        (doubles)
// with a FIXED stride VWS_GS between the 4-point k-groups.  A fragment read of k-group kk is then  ds_read_b64 v, addr
// offset:kk*VWS_GS*8  with one per-tile address register that does not change within a chunk: no VALU instruction at
// all between the MFMAs.  (With the natural stride 4 * ld, a run-time value, every read needs a v_add first; those two
// VALU instructions per MFMA cost 16 % of the MFMA rate -- tools/ubench/barrier_cost.hip: 60.6 vs 72.2 TF.)
constexpr int VWS_LSMAX = 256;                    // LS <= 256, i.e. ld <= 240 (T <= 15), reaches this layout (wider: vxc_ws2_kernel)
constexpr int VWS_GS = 4 * VWS_LSMAX;             // doubles between k-groups
constexpr int VWS_XS = (16 / 4) * VWS_GS;         // doubles between Phi and Psi (16-point chunks)
constexpr int VWS_BUF = 2 * VWS_XS;               // doubles per buffer: 64 KB; two buffers = 128 KB of the 160 KB
typedef const __attribute__((address_space(3))) double lds_cdouble_t;
// vxc_ws2_kernel (rectangles of at most 8 x 11 tiles): Phi rows <= 8*16 (+16 pad), Psi rows <= 11*16 (+16 pad)
constexpr int WS2_GSA = 4 * 144, WS2_GSB = 4 * 208;       // k-group strides (doubles)
constexpr int WS2_XS = 4 * WS2_GSA;                       // Phi part -> Psi part
constexpr int WS2_BUF = WS2_XS + 4 * WS2_GSB;             // doubles per buffer (44 KB)

// One chunk of a consumer wave: (KCH / 4) k-steps x MAXT tiles of fragment reads + MFMAs, SOFTWARE-PIPELINED by hand.  Left
// to itself the compiler emits  ds_read a; ds_read b; s_waitcnt lgkmcnt(0); v_mfma  per tile (it minimises fragment
// registers), which exposes the LDS latency in front of every MFMA; here the fragments of step s + D are requested
// before the MFMA of step s and sched_barriers pin that order.  pa / pb: LDS byte addresses of the tile's A / B fragment
// in k-group 0 of the current buffer.
#ifndef WS_D
#define WS_D 2
#endif
template <int MAXT, int KCH, int D = WS_D, int GSA = VWS_GS, int GSB = VWS_GS, int NTL = MAXT>
__device__ __forceinline__ void ws_chunk(const unsigned (&pa)[MAXT], const unsigned (&pb)[MAXT], v4d (&acc)[MAXT]) {
    // NTL <= MAXT: the tiles this wave really owns (no dummy MFMAs: the deal below gives the waves of a block tile counts
    // that differ by at most one, and every count has its own straight-line body)
    constexpr int NS = (KCH / 4) * NTL;
    if constexpr (NTL > 0) {
        double fa[D + 1], fb[D + 1];
#pragma unroll
        for (int s = 0; s < D && s < NS; s++) {
            fa[s % (D + 1)] = *(lds_cdouble_t *)(pa[s % NTL] + (s / NTL) * GSA * 8);
            fb[s % (D + 1)] = *(lds_cdouble_t *)(pb[s % NTL] + (s / NTL) * GSB * 8);
        }
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (s + D < NS) {
                const int s2 = s + D;
                fa[s2 % (D + 1)] = *(lds_cdouble_t *)(pa[s2 % NTL] + (s2 / NTL) * GSA * 8);
                fb[s2 % (D + 1)] = *(lds_cdouble_t *)(pb[s2 % NTL] + (s2 / NTL) * GSB * 8);
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[s % NTL] = mfma_f64(fa[s % (D + 1)], fb[s % (D + 1)], acc[s % NTL]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
// A consumer wave of vxc_ws_kernel / vxc_ws2_kernel with NTL tiles (compile time: the accumulators, the fragment addresses and
// the straight-line MFMA stream are sized for exactly the tiles the wave owns).  Tile u = t0 + t of the block's list maps to
// local tile coordinates (li, lj) -- LDS columns 16 li of the A part, 16 lj of the B part -- and to the output tile
// (r0 + li, c0 + lj):  nc > 0: rectangle, (u / nc, u % nc);  nc == 0, sym == 0: (u / T, u % T);  sym: upper triangle of T rows.
struct WsTiles { int sym, T, nc, r0, c0, t0, nreal; };  // nreal: tiles of the block's list that exist (vxc_ws2_kernel pads lighter blocks)
__device__ __forceinline__ void ws_tile(const WsTiles &m, int u, int &li, int &lj) {
    if (m.nc) { li = u / m.nc; lj = u - li * m.nc; return; }
    if (!m.sym) { li = u / m.T; lj = u - li * m.T; return; }
    int i = 0, rem = u;
    while (rem >= m.T - i) { rem -= m.T - i; i++; }  // row i of the upper triangle holds T - i tiles
    li = i;
    lj = i + rem;
}
template <int NTL, int KCH, int D, int GSA, int GSB, int XS, int BUF>
__device__ __forceinline__ void ws_consumer(double *lds, double *__restrict__ vmat, int ld, int nchunk, const WsTiles m, int LSA, int LSB) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    constexpr int NA = NTL > 0 ? NTL : 1;
    v4d acc[NA];
    unsigned pa[NA], pb[NA];  // LDS byte addresses of the A / B fragments (k-group 0, current buffer)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds;
#pragma unroll
    for (int t = 0; t < NTL; t++) {
        acc[t] = v4d{0, 0, 0, 0};
        int li, lj;
        ws_tile(m, min(m.t0 + t, m.nreal - 1), li, lj);  // (a padding tile re-reads the block's last one; its sum is discarded)
        pa[t] = lds0 + 8u * (unsigned)(lk * LSA + li * 16 + lr);
        pb[t] = lds0 + 8u * (unsigned)(XS + lk * LSB + lj * 16 + lr);
    }
    __syncthreads();
    for (int c = 0; c < nchunk; c++) {
        __syncthreads();  // chunk c - 1 done: the producers' combine window opens ...
        __syncthreads();  // ... and closes
        if constexpr (NTL > 0) {
            ws_chunk<NA, KCH, D, GSA, GSB, NTL>(pa, pb, acc);
            const unsigned delta = (c & 1) ? (unsigned)(-BUF * 8) : (unsigned)(BUF * 8);  // on to the other buffer
#pragma unroll
            for (int t = 0; t < NTL; t++) { pa[t] += delta; pb[t] += delta; }
        }
    }
#pragma unroll
    for (int t = 0; t < NTL; t++) {
        if (m.t0 + t >= m.nreal) continue;
        int li, lj;
        ws_tile(m, m.t0 + t, li, lj);
        const int ia = (m.r0 + li) * 16 + lk, ib = (m.c0 + lj) * 16 + lr;
        const double sc = (m.sym && li != lj) ? 2.0 : 1.0;
#pragma unroll
        for (int r = 0; r < 4; r++) acc_add(&vmat[(size_t)(ia + 4 * r) * ld + ib], sc * acc[t][r], g_vxc_det_scale);
    }
}
// dispatch on the (wave-uniform) tile count nt in [0, MAXT]
template <int MAXT, int KCH, int D, int GSA, int GSB, int XS, int BUF, int N = MAXT>
__device__ __forceinline__ void ws_consumer_n(int nt, double *lds, double *__restrict__ vmat, int ld, int nchunk, const WsTiles m,
                                              int LSA, int LSB) {
    if (nt == N) ws_consumer<N, KCH, D, GSA, GSB, XS, BUF>(lds, vmat, ld, nchunk, m, LSA, LSB);
    else if constexpr (N > 0) ws_consumer_n<MAXT, KCH, D, GSA, GSB, XS, BUF, N - 1>(nt, lds, vmat, ld, nchunk, m, LSA, LSB);
}
// balanced deal of `n` tiles to the 8 consumer waves: counts differ by at most one (waves w and w + 4 share a SIMD)
__device__ __forceinline__ void ws_deal(int n, int wave, int &t0, int &nt) {
    const int tbase = n / VXC_WAVES, trem = n % VXC_WAVES;
    nt = tbase + (wave < trem ? 1 : 0);
    t0 = wave * tbase + min(wave, trem);
}

template <int MAXT, int NLP, int KCH, bool GGA>
__global__ __launch_bounds__(VWS_NT, VWS_NT / 256) void vxc_ws_kernel(double *__restrict__ vmat, const double *__restrict__ ao,
                                                          int ngrid, int ld, const double *__restrict__ w,
                                                          const double *__restrict__ vrho,
                                                          const double *__restrict__ vgrad, int slab, int nsplit,
                                                          int tiles_per_split, const double *__restrict__ aob, int sym, int lda, int LS) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    static_assert(KCH == 16, "the fixed-stride chunk layout is laid out for 16-point chunks");
    constexpr int BUF = VWS_BUF;  // (lda / ld / LS: see the head of the file)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t cs = (size_t)ngrid * lda;
    const int id = blockIdx.x;
    const int grp = id / (8 * nsplit), rem = id - grp * 8 * nsplit;
    const int split = rem / 8, sl = grp * 8 + (rem & 7);
    const int gs = sl * slab, ge = min(gs + slab, ngrid);
    if (gs >= ngrid) return;
    const int nchunk = (ge - gs + KCH - 1) / KCH;

    if (wave >= VXC_WAVES) {
        // ------------------------------------------------------------------ producers
        __builtin_amdgcn_s_setprio(3);  // the fp64 combine shares the DP pipe with the consumers' MFMAs: win arbitration
        // Measured (tools/ubench/vxc_trace.hip): an fp64 MFMA occupies the SIMD's vector ALU for its 64 cycles, and against two
        // waves issuing MFMAs back to back every VALU instruction of a third wave waits for a whole MFMA -- a producer that
        // needs ~250 VALU instructions per chunk (address arithmetic, selects, the combine) then takes twice the MFMA time.
        // The producer loop is therefore written to need almost no VALU work outside the combine:
        //   * global loads in  SGPR base + one loop-invariant VGPR offset + immediate  form (the chunk / component base
        //     advances on the scalar unit),
        //   * LDS writes as one address register + immediates,
        //   * the tail chunk (rows past the slab end) on a separate, wave-uniform path.
        constexpr int TPR = VWS_PROD / KCH;  // threads per chunk row
        const int pt = tid - 512;
        const int prow = pt / TPR, pcol = pt % TPR;
        const unsigned voff0 = 8u * (unsigned)(prow * lda + pcol * 2);  // bytes from the chunk's first row
        unsigned wlds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds +
                        8u * (unsigned)((prow >> 2) * VWS_GS + (prow & 3) * LS + pcol * 2);  // Phi slot in buffer 0
        typedef double vd2 __attribute__((ext_vector_type(2)));
        //     Buffer loads give exactly that addressing, and their range check (num_records = bytes left in the slab) returns
        //     zeros for rows past the slab end: Phi = Psi = w = 0 there, no per-lane row guard anywhere.
        typedef unsigned int v4u __attribute__((ext_vector_type(4)));
        typedef unsigned int v2u __attribute__((ext_vector_type(2)));
        constexpr int BUF_FLAGS = 0x00020000;  // raw buffer, 32-bit data format (gfx9 dword 3)
        v4u raw[NLP][GGA ? 4 : 2];
        double cf[GGA ? 4 : 1], wg = 0.0;
        auto as_d = [](unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); };
        auto prefetch = [&](int c) {
            const int g0 = gs + c * KCH;                 // uniform: everything below but voff0 / prow lives in SGPRs
            const int rows = ge - g0;                    // rows left in the slab (> 0)
            auto rsrc = [&](const double *base, size_t bytes) {
                return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)bytes, BUF_FLAGS);
            };
            const v2u xw = __builtin_amdgcn_raw_buffer_load_b64(rsrc(w + g0, (size_t)rows * 8), prow * 8, 0, 0);
            wg = as_d(xw[0], xw[1]);
            const v2u xr = __builtin_amdgcn_raw_buffer_load_b64(rsrc(vrho + g0, (size_t)rows * 8), prow * 8, 0, 0);
            cf[0] = as_d(xr[0], xr[1]);
            if (GGA) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const v2u xg = __builtin_amdgcn_raw_buffer_load_b64(rsrc(vgrad + (size_t)d * ngrid + g0, (size_t)rows * 8), prow * 8, 0, 0);
                    cf[d + 1] = as_d(xg[0], xg[1]);
                }
            }
            const size_t nb = (size_t)rows * lda * 8;    // < 2^31: a slab is a few MB
#pragma unroll
            for (int d = 0; d < (GGA ? 4 : 1); d++) {
                const auto r = rsrc(ao + d * cs + (size_t)g0 * lda, nb);
#pragma unroll
                for (int i = 0; i < NLP; i++)
                    if ((pcol + i * TPR) * 2 < ld) raw[i][d] = __builtin_amdgcn_raw_buffer_load_b128(r, voff0 + i * TPR * 16, 0, 0);
            }
            if (!GGA && !sym) {  // (sym: the second operand is the first)
                const auto r = rsrc(aob + (size_t)g0 * lda, nb);
#pragma unroll
                for (int i = 0; i < NLP; i++)
                    if ((pcol + i * TPR) * 2 < ld) raw[i][1] = __builtin_amdgcn_raw_buffer_load_b128(r, voff0 + i * TPR * 16, 0, 0);
            }
        };
        auto stage = [&]() {  // Psi from the raw registers; (Phi, Psi) -> the buffer wlds points into
            cf[0] *= wg;
            if (GGA) {
#pragma unroll
                for (int d = 1; d < 4; d++) cf[d] *= 2.0 * wg;
            }
#pragma unroll
            for (int i = 0; i < NLP; i++) {
                if ((pcol + i * TPR) * 2 < ld) {
                    const v4u pb = (GGA || sym) ? raw[i][0] : raw[i][1];
                    vd2 ps = {cf[0] * as_d(pb[0], pb[1]), cf[0] * as_d(pb[2], pb[3])};
                    if (GGA) {
#pragma unroll
                        for (int d = 1; d < 4; d++) {
                            ps.x += cf[d] * as_d(raw[i][d][0], raw[i][d][1]);
                            ps.y += cf[d] * as_d(raw[i][d][2], raw[i][d][3]);
                        }
                    }
                    *(__attribute__((address_space(3))) v4u *)(wlds + i * TPR * 16) = raw[i][0];
                    *(__attribute__((address_space(3))) vd2 *)(wlds + i * TPR * 16 + VWS_XS * 8) = ps;
                }
            }
        };
        prefetch(0);
        stage();
        if (nchunk > 1) prefetch(1);
        __syncthreads();
        if (wave == VXC_WAVES) VXC_TRACE_POINT(1, 0);
        for (int c = 0; c < nchunk; c++) {
            wlds += (c & 1) ? (unsigned)(-VWS_BUF * 8) : (unsigned)(VWS_BUF * 8);  // buffer (c + 1) & 1
            __syncthreads();  // the consumers have finished chunk c - 1 and wait: the vector ALUs are free for the combine
            if (c + 1 < nchunk) stage();              // chunk c + 1: its loads were issued a whole period ago
            if (wave == VXC_WAVES) VXC_TRACE_POINT(1, c + 1);  // combine done
            __syncthreads();  // the consumers start the MFMAs of chunk c
            if (c + 2 < nchunk) prefetch(c + 2);      // VALU-free issue, in flight during the MFMAs
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers
    // sym: A^T diag(w v) A with ONE operand (LDA Vxc, the tau terms of a meta-GGA) is symmetric -- only the tiles (i <= j) are
    // computed, off-diagonal ones doubled so that the final (M + M^T) / 2 restores both halves
    const int T = ld >> 4, ttot = sym ? T * (T + 1) / 2 : T * T;
    const int tc0 = split * tiles_per_split;
    const int tc1 = min(tc0 + tiles_per_split, ttot);
    int t0, nt;
    ws_deal(tc1 - tc0, wave, t0, nt);
    const WsTiles m{sym, T, 0, 0, 0, tc0 + t0, tc1};
    ws_consumer_n<MAXT, KCH, WS_D, VWS_GS, VWS_GS, VWS_XS, VWS_BUF>(nt, lds, vmat, ld, nchunk, m, LS, LS);
}

// ---------------------------------------------------------------------------------------------
// Vxc for larger bases: the wave-specialised kernel with RECTANGULAR output ownership.  vxc_ws_kernel splits the
// T x T output tiles linearly over `nsplit` blocks that each stage ALL columns of a slab; beyond two blocks per
// slab that re-reads the slab nsplit times (nsplit = 18 at nao = 624).  Here block (slab, i, j) owns the tile
// rectangle  rows [i T / NR, (i+1) T / NR)  x  cols [j T / NC, (j+1) T / NC)  (<= 9 x 12 tiles, <= 88 of them) and its producers
// stage only the Phi columns of those rows (A operand) and the four AO components of those columns (-> Psi, B
// operand): per-block loads are what vxc_ws_kernel loads at nao = 208, and a slab is re-read NC + 4 NR times in
// total instead of 5 nsplit.  Chunks are always 16 points (39 KB per LDS buffer).
// ---------------------------------------------------------------------------------------------
template <int MAXT, int NLA, int NLB, bool GGA>
__global__ __launch_bounds__(VWS2_NT, 3) void vxc_ws2_kernel(double *__restrict__ vmat, const double *__restrict__ ao,
                                                           int ngrid, int ld, const double *__restrict__ w,
                                                           const double *__restrict__ vrho,
                                                           const double *__restrict__ vgrad, int slab, int NR, int NC,
                                                           int LSA, int LSB, const double *__restrict__ aob, int lda) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int KCH = 16;
    // chunk layout as in vxc_ws_kernel: fixed strides between the 4-point k-groups (Phi part: WS2_GSA, Psi part: WS2_GSB), so that
    // the consumers' fragment reads are  address register + immediate;  rows inside a k-group at the run-time strides LSA / LSB
    constexpr int BUF = WS2_BUF;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t cs = (size_t)ngrid * lda;
    const int T = ld >> 4, nsplit = NR * NC;
    const int id = blockIdx.x;
    const int grp = id / (8 * nsplit), rem = id - grp * 8 * nsplit;
    const int split = rem / 8, sl = grp * 8 + (rem & 7);
    const int gs = sl * slab, ge = min(gs + slab, ngrid);
    if (gs >= ngrid) return;
    const int nchunk = (ge - gs + KCH - 1) / KCH;
    const int bi = split / NC, bj = split % NC;
    const int r0 = bi * T / NR, nr = (bi + 1) * T / NR - r0;   // tile rows of this block
    const int c0 = bj * T / NC, nc = (bj + 1) * T / NC - c0;   // tile columns
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds;

    if (wave >= VXC_WAVES) {
        // ------------------------------------------------------------------ producers (see vxc_ws_kernel: buffer loads with
        // SGPR base + loop-invariant VGPR offset + immediate, range-checked against the slab end; the combine in its own window)
        __builtin_amdgcn_s_setprio(3);
        constexpr int TPR = VWS2_PROD / KCH;  // 16 threads per chunk row
        const int pt = tid - 512;
        const int prow = pt / TPR, pcol = pt % TPR;
        const int wa = nr * 16, wb = nc * 16;  // staged widths (doubles)
        const unsigned voff0 = 8u * (unsigned)(prow * lda + pcol * 2);
        unsigned wla = lds0 + 8u * (unsigned)((prow >> 2) * WS2_GSA + (prow & 3) * LSA + pcol * 2);
        unsigned wlb = lds0 + 8u * (unsigned)(WS2_XS + (prow >> 2) * WS2_GSB + (prow & 3) * LSB + pcol * 2);
        typedef unsigned int v4u __attribute__((ext_vector_type(4)));
        typedef unsigned int v2u __attribute__((ext_vector_type(2)));
        typedef double vd2 __attribute__((ext_vector_type(2)));
        constexpr int BUF_FLAGS = 0x00020000;
        v4u ra[NLA], rb[NLB][GGA ? 4 : 1];
        double cf[GGA ? 4 : 1], wg = 0.0;
        auto as_d = [](unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); };
        auto prefetch = [&](int c) {
            const int g0 = gs + c * KCH;
            const int rows = ge - g0;
            auto rsrc = [&](const double *base, size_t bytes) {
                return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)bytes, BUF_FLAGS);
            };
            const v2u xw = __builtin_amdgcn_raw_buffer_load_b64(rsrc(w + g0, (size_t)rows * 8), prow * 8, 0, 0);
            wg = as_d(xw[0], xw[1]);
            const v2u xr = __builtin_amdgcn_raw_buffer_load_b64(rsrc(vrho + g0, (size_t)rows * 8), prow * 8, 0, 0);
            cf[0] = as_d(xr[0], xr[1]);
            if (GGA) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const v2u xg = __builtin_amdgcn_raw_buffer_load_b64(rsrc(vgrad + (size_t)d * ngrid + g0, (size_t)rows * 8), prow * 8, 0, 0);
                    cf[d + 1] = as_d(xg[0], xg[1]);
                }
            }
            // bytes from the rectangle's first column of row g0 to the end of the slab (the loads of a row stop at its staged width)
            const size_t nba = (size_t)rows * lda * 8 - (size_t)r0 * 128, nbb = (size_t)rows * lda * 8 - (size_t)c0 * 128;
            {
                const auto r = rsrc(ao + (size_t)g0 * lda + r0 * 16, nba);
#pragma unroll
                for (int i = 0; i < NLA; i++)
                    if ((pcol + i * TPR) * 2 < wa) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(r, voff0 + i * TPR * 16, 0, 0);
            }
#pragma unroll
            for (int d = 0; d < (GGA ? 4 : 1); d++) {
                const auto r = rsrc((GGA ? ao : aob) + d * cs + (size_t)g0 * lda + c0 * 16, nbb);
#pragma unroll
                for (int i = 0; i < NLB; i++)
                    if ((pcol + i * TPR) * 2 < wb) rb[i][d] = __builtin_amdgcn_raw_buffer_load_b128(r, voff0 + i * TPR * 16, 0, 0);
            }
        };
        auto stage = [&]() {
            cf[0] *= wg;
            if (GGA) {
#pragma unroll
                for (int d = 1; d < 4; d++) cf[d] *= 2.0 * wg;
            }
#pragma unroll
            for (int i = 0; i < NLA; i++)
                if ((pcol + i * TPR) * 2 < wa) *(__attribute__((address_space(3))) v4u *)(wla + i * TPR * 16) = ra[i];
#pragma unroll
            for (int i = 0; i < NLB; i++) {
                if ((pcol + i * TPR) * 2 < wb) {
                    vd2 ps = {cf[0] * as_d(rb[i][0][0], rb[i][0][1]), cf[0] * as_d(rb[i][0][2], rb[i][0][3])};
                    if (GGA) {
#pragma unroll
                        for (int d = 1; d < 4; d++) {
                            ps.x += cf[d] * as_d(rb[i][d][0], rb[i][d][1]);
                            ps.y += cf[d] * as_d(rb[i][d][2], rb[i][d][3]);
                        }
                    }
                    *(__attribute__((address_space(3))) vd2 *)(wlb + i * TPR * 16) = ps;
                }
            }
        };
        prefetch(0);
        stage();
        if (nchunk > 1) prefetch(1);
        __syncthreads();
        for (int c = 0; c < nchunk; c++) {
            const unsigned delta = (c & 1) ? (unsigned)(-BUF * 8) : (unsigned)(BUF * 8);  // buffer (c + 1) & 1
            wla += delta;
            wlb += delta;
            __syncthreads();  // the consumers have finished chunk c - 1 and wait: the vector ALUs are free for the combine
            if (c + 1 < nchunk) stage();
            __syncthreads();  // the consumers start the MFMAs of chunk c
            if (c + 2 < nchunk) prefetch(c + 2);
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers
    // EVERY block of a slab runs the tile count of the largest rectangle (the smaller ones pad with repeats of their last tile):
    // blocks that issue the same MFMA stream per chunk walk through the slab in step, and the slab's rows then come out of
    // the XCD's L2 for all but the first reader.  With the exact counts (T = 26: 64 ... 81 tiles) the lighter blocks ran ahead and
    // FETCH_SIZE doubled (9.7 instead of 4.9 GB per launch at nao 412) for the same launch time
    const int ntmax = ((T + NR - 1) / NR) * ((T + NC - 1) / NC);
    int t0, nt;
    ws_deal(ntmax, wave, t0, nt);
    const WsTiles m{0, T, nc, r0, c0, t0, nr * nc};
    ws_consumer_n<MAXT, KCH, 4, WS2_GSA, WS2_GSB, WS2_XS, WS2_BUF>(nt, lds, vmat, ld, nchunk, m, LSA, LSB);
}

// ---------------------------------------------------------------------------------------------
// Vxc, ONE block per slab (bases with 10 <= T <= 13 tile rows, i.e. 145 <= nao <= 208: the 20-atom cc-pVDZ molecules).
// vxc_ws_kernel needs two blocks per slab there (T^2 = 169 tiles > 8 waves x 11), so every chunk travels L2 -> CU twice
// and the chunk period is set by the producers' loads (2.7 us), not by the MFMAs (2.5 us).  Here the block owns the
// UPPER-TRIANGULAR tiles only (T (T + 1) / 2 = 91 <= 8 x 12) and accumulates the symmetrised matrix directly.  Two kernels
// share the scheme, the producer (vwu_producer) and the block shape (8 consumer + 4 producer waves, one producer per SIMD):
//     vxc_wsu_kernel (here):   one operand, no gradient term -- M is symmetric:   acc_ij = Phi_i^T Psi_j = M_ij = V_ij,
//                              one MFMA per tile and k-group, T (T + 1) / 2 of them instead of T^2
//     vxc_wsd_kernel (below):  GGA:   acc_ij = Phi_i^T Psi_j + Psi_i^T Phi_j = M_ij + (M_ji)^T = 2 V_ij  on the off-diagonal tiles
//                              (its figures: the comment above that kernel)
// Against two blocks per slab: half the L2 -> CU traffic, half the producers and one combine window per 2 x the MFMA work.
// Chunk layout, buffer loads, the two-barrier combine window and the hand-pipelined fragment reads are those of
// vxc_ws_kernel; the fragment of tile row i is  Phi: pi[t] + kk GS 8,  Psi: pi[t] + (XS + kk GS) 8  (immediates).
// ---------------------------------------------------------------------------------------------
constexpr int VWU_PROD = 256, VWU_NT = 512 + VWU_PROD;

#ifdef VWU_TRACE  // per-chunk timeline of one block (100 MHz ticks): role 0 = consumer wave 0, role 1 = producer wave 8
constexpr int VWU_TRACE_N = 4 * 128;
__device__ long long g_vwu_trace[2 * VWU_TRACE_N];
#define VWU_STAMP(role, slot) \
    if (blockIdx.x == VWU_TRACE && (wave == 0 || wave == 8) && lane == 0 && (slot) < VWU_TRACE_N) g_vwu_trace[(role) * VWU_TRACE_N + (slot)] = wall_clock64()
#else
#define VWU_STAMP(role, slot)
#endif

template <int MAXT, int NTL, int D = 2>
__device__ __forceinline__ void wsu_chunk(const unsigned (&pi)[MAXT], const unsigned (&pj)[MAXT], v4d (&acc)[MAXT]) {
    // NTL <= MAXT: tiles actually looped over (waves that own one tile fewer skip the dummy MFMAs); step s: k-group s / NTL of
    // the 16-point chunk, tile s % NTL:  A = Phi_i, B = Psi_j
    constexpr int NS = 4 * NTL;
    double fa[D + 1], fb[D + 1];
    auto rd = [&](int s) {
        fa[s % (D + 1)] = *(lds_cdouble_t *)(pi[s % NTL] + (s / NTL) * VWS_GS * 8);
        fb[s % (D + 1)] = *(lds_cdouble_t *)(pj[s % NTL] + ((s / NTL) * VWS_GS + VWS_XS) * 8);
    };
#pragma unroll
    for (int s = 0; s < D && s < NS; s++) rd(s);
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s + D < NS) rd(s + D);
        __builtin_amdgcn_sched_barrier(0);
        acc[s % NTL] = mfma_f64(fa[s % (D + 1)], fb[s % (D + 1)], acc[s % NTL]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the same with a (wave-uniform) run-time tile count in [0, MAXT]: one straight-line body per count, no dummy MFMAs
template <int MAXT, int N = MAXT>
__device__ __forceinline__ void wsu_chunk_n(int nt, const unsigned (&pi)[MAXT], const unsigned (&pj)[MAXT], v4d (&acc)[MAXT]) {
    if constexpr (N == 0) return;
    else if (nt == N) wsu_chunk<MAXT, N>(pi, pj, acc);
    else wsu_chunk_n<MAXT, N - 1>(nt, pi, pj, acc);
}

// the 4 producer waves of vxc_wsu_kernel / vxc_wsd_kernel (threads 512 .. 767): chunk c + 2 travels HBM -> registers while the
// consumers run the MFMAs of chunk c; chunk c + 1 is combined into (Phi, Psi) and written to LDS in the window between chunks
template <int NLP, bool GGA>
DQC_DEV void vwu_producer(double *lds, const double *__restrict__ ao, int ngrid, int ld, const double *__restrict__ w,
                          const double *__restrict__ vrho, const double *__restrict__ vgrad, int gs, int ge, int nchunk,
                          int lda, int LS) {
    // lda: row stride of the AO arrays in HBM; ld = 16 T: staged width; LS: LDS row stride (see the head of the file)
    constexpr int KCH = 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    (void)wave; (void)lane;
    const size_t cs = (size_t)ngrid * lda;
    // ------------------------------------------------------------------ producers (see vxc_ws_kernel)
    __builtin_amdgcn_s_setprio(3);
    constexpr int TPR = VWU_PROD / KCH;  // 16 threads per chunk row
    const int pt = tid - 512;
    const int prow = pt / TPR, pcol = pt % TPR;
    const unsigned voff0 = 8u * (unsigned)(prow * lda + pcol * 2);
    unsigned wlds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds +
                    8u * (unsigned)((prow >> 2) * VWS_GS + (prow & 3) * LS + pcol * 2);
    typedef double vd2 __attribute__((ext_vector_type(2)));
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    typedef unsigned int v2u __attribute__((ext_vector_type(2)));
    constexpr int BUF_FLAGS = 0x00020000;
    v4u raw[NLP][GGA ? 4 : 1];
    double cf[GGA ? 4 : 1], wg = 0.0;
    auto as_d = [](unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); };
    auto prefetch = [&](int c) {
        const int g0 = gs + c * KCH;
        const int rows = ge - g0;
        auto rsrc = [&](const double *base, size_t bytes) {
            return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)bytes, BUF_FLAGS);
        };
        const v2u xw = __builtin_amdgcn_raw_buffer_load_b64(rsrc(w + g0, (size_t)rows * 8), prow * 8, 0, 0);
        wg = as_d(xw[0], xw[1]);
        const v2u xr = __builtin_amdgcn_raw_buffer_load_b64(rsrc(vrho + g0, (size_t)rows * 8), prow * 8, 0, 0);
        cf[0] = as_d(xr[0], xr[1]);
        if (GGA) {
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const v2u xg = __builtin_amdgcn_raw_buffer_load_b64(rsrc(vgrad + (size_t)d * ngrid + g0, (size_t)rows * 8), prow * 8, 0, 0);
                cf[d + 1] = as_d(xg[0], xg[1]);
            }
        }
        const size_t nb = (size_t)rows * lda * 8;
#pragma unroll
        for (int d = 0; d < (GGA ? 4 : 1); d++) {
            const auto r = rsrc(ao + d * cs + (size_t)g0 * lda, nb);
#pragma unroll
            for (int i = 0; i < NLP; i++)
                if ((pcol + i * TPR) * 2 < ld) raw[i][d] = __builtin_amdgcn_raw_buffer_load_b128(r, voff0 + i * TPR * 16, 0, 0);
        }
    };
    auto stage = [&]() {
        // GGA: acc = 2 V, so Psi = w (vrho Phi + sum_d 2 vgrad_d dPhi_d) as in vxc_ws_kernel and the epilogue halves
        cf[0] *= wg;
        if (GGA) {
#pragma unroll
            for (int d = 1; d < 4; d++) cf[d] *= 2.0 * wg;
        }
#pragma unroll
        for (int i = 0; i < NLP; i++) {
            if ((pcol + i * TPR) * 2 < ld) {
                vd2 ps = {cf[0] * as_d(raw[i][0][0], raw[i][0][1]), cf[0] * as_d(raw[i][0][2], raw[i][0][3])};
                if (GGA) {
#pragma unroll
                    for (int d = 1; d < 4; d++) {
                        ps.x += cf[d] * as_d(raw[i][d][0], raw[i][d][1]);
                        ps.y += cf[d] * as_d(raw[i][d][2], raw[i][d][3]);
                    }
                }
                *(__attribute__((address_space(3))) v4u *)(wlds + i * TPR * 16) = raw[i][0];
                *(__attribute__((address_space(3))) vd2 *)(wlds + i * TPR * 16 + VWS_XS * 8) = ps;
            }
        }
    };
    prefetch(0);
    stage();
    if (nchunk > 1) prefetch(1);
    __syncthreads();
#ifdef VWU_TRACE
    if (blockIdx.x == VWU_TRACE && tid == 512) { g_vwu_trace[VWU_TRACE_N - 4] = clock64(); g_vwu_trace[VWU_TRACE_N - 3] = wall_clock64(); }
#endif
    for (int c = 0; c < nchunk; c++) {
        wlds += (c & 1) ? (unsigned)(-VWS_BUF * 8) : (unsigned)(VWS_BUF * 8);  // buffer (c + 1) & 1
        __syncthreads();  // the consumers have finished chunk c - 1 and wait: the vector ALUs are free for the combine
#ifdef VWU_TRACE_CHUNKS
        VWU_STAMP(1, 4 * c);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        VWU_STAMP(1, 4 * c + 1);
#endif
#ifndef VWU_EXP_NOSTAGE
        if (c + 1 < nchunk) stage();
#endif
        __syncthreads();  // the consumers start the MFMAs of chunk c
#ifndef VWU_EXP_NOLOAD
        if (c + 2 < nchunk) prefetch(c + 2);
#endif
    }
#ifdef VWU_TRACE
    if (blockIdx.x == VWU_TRACE && tid == 512) { g_vwu_trace[VWU_TRACE_N - 2] = clock64(); g_vwu_trace[VWU_TRACE_N - 1] = wall_clock64(); }
#endif
}

template <int MAXT, int NLP>
__global__ __launch_bounds__(VWU_NT, 3) void vxc_wsu_kernel(double *__restrict__ vmat, const double *__restrict__ ao, int ngrid,
                                                           int ld, const double *__restrict__ w, const double *__restrict__ vrho,
                                                           const double *__restrict__ vgrad, int slab, int lda, int LS) {
    // (vgrad: not read -- no gradient term in this form; the launcher passes it through for a uniform argument list)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int KCH = 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gs = blockIdx.x * slab, ge = min(gs + slab, ngrid);
    if (gs >= ngrid) return;
    const int nchunk = (ge - gs + KCH - 1) / KCH;

    if (wave >= VXC_WAVES) {
        vwu_producer<NLP, false>(lds, ao, ngrid, ld, w, vrho, vgrad, gs, ge, nchunk, lda, LS);
        return;
    }

    // ---------------------------------------------------------------------- consumers: upper-triangular tiles
    const int lr = lane & 15, lk = lane >> 4;
    const int T = ld >> 4, ttot = T * (T + 1) / 2;
    auto tile_ij = [&](int u, int &ti, int &tj) {
        int i = 0, rem = u;
        while (rem >= T - i) { rem -= T - i; i++; }  // row i of the upper triangle holds T - i tiles
        ti = i;
        tj = i + rem;
    };
    // balanced deal: the first ttot % 8 waves own one tile more.  Waves w and w + 4 share a SIMD (a block's waves go to the
    // SIMDs cyclically), so for T = 13 the SIMDs carry 23, 23, 23, 22 tiles and no dummy MFMA is issued
    const int tbase = ttot / VXC_WAVES, trem = ttot % VXC_WAVES;
    const int nt = tbase + (wave < trem ? 1 : 0);
    const int t0 = wave * tbase + min(wave, trem);
    v4d acc[MAXT];
    unsigned pi[MAXT], pj[MAXT];  // LDS byte addresses of the row / column fragments in the Phi part (k-group 0, current buffer)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds;
#pragma unroll
    for (int t = 0; t < MAXT; t++) {
        acc[t] = v4d{0, 0, 0, 0};
        int ti, tj;
        tile_ij(min(t0 + min(t, max(nt - 1, 0)), ttot - 1), ti, tj);
        pi[t] = lds0 + 8u * (unsigned)(lk * LS + ti * 16 + lr);
        pj[t] = lds0 + 8u * (unsigned)(lk * LS + tj * 16 + lr);
    }
    __syncthreads();
    for (int c = 0; c < nchunk; c++) {
#ifdef VWU_TRACE_CONS
        VWU_STAMP(0, 4 * c);
#endif
        __syncthreads();  // chunk c - 1 done: the producers' combine window opens ...
        __syncthreads();  // ... and closes
#ifdef VWU_TRACE_CONS
        VWU_STAMP(0, 4 * c + 1);
#endif
#ifndef VWU_EXP_NOMFMA
        wsu_chunk_n<MAXT>(nt, pi, pj, acc);
#endif
        const unsigned delta = (c & 1) ? (unsigned)(-VWS_BUF * 8) : (unsigned)(VWS_BUF * 8);
#pragma unroll
        for (int t = 0; t < MAXT; t++) { pi[t] += delta; pj[t] += delta; }
    }
#pragma unroll
    for (int t = 0; t < MAXT; t++) {
        if (t < nt) {
            int ti, tj;
            tile_ij(t0 + t, ti, tj);
            const int ia = ti * 16 + lk, ib = tj * 16 + lr;
            // symmetrize_kernel forms (m_ij + m_ji) / 2 over the whole matrix and the lower tiles stay zero:
            // acc = V -> off-diagonal tiles store 2 acc, diagonal tiles acc
            const double sc = ti != tj ? 2.0 : 1.0;
#ifdef VWU_EXP_NOEPI
            if (acc[t][0] != 1.2345e300) continue;
#endif
#pragma unroll
            for (int r = 0; r < 4; r++) acc_add(&vmat[(size_t)(ia + 4 * r) * ld + ib], sc * acc[t][r], g_vxc_det_scale);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Vxc, one block per slab, GGA, 10 <= T <= 13 tile rows: the upper-triangular scheme with two MFMAs on the off-diagonal tiles
// and ONE on the diagonal tiles.  With two on every tile the kernel is 90 % MFMA-busy in cycles, but the chip sits at its
// power limit there (tools/gpu_vxc_trace.py: the shader clock is 1.96 GHz with the MFMAs and the HBM stream both running,
// 2.35 GHz with the MFMAs alone, 2.41 GHz with the stream alone), so what is left is the number of MFMAs.  A diagonal tile
// needs only M_ii = Phi_i^T Psi_i: symmetrize_kernel forms (M_ii + M_ii^T) / 2 = V_ii anyway.  T^2 = 169 MFMAs per k-group
// instead of T (T + 1) = 182 (-7 %) -- as many as the two-block vxc_ws_kernel form issues.  12 waves per block => 168 VGPRs
// per wave for the 12 accumulator tiles.  Measured (C5 shape, random data): 0.691 ms against 0.725 ms.
//
// Fragment reuse.  The A fragment of tile row t and the B fragment of tile column t are the same 64 doubles in the same
// lanes (LDS doubles lk LS + 16 t + lr of the component), so a fragment is named by (Phi or Psi, tile index t, k-group)
// alone and a wave that owns the tile set S needs, per k-group, the 2 |U| fragments of the tile indices U that occur in S
// as a row or as a column -- however many MFMAs use them.  The ownership (WSD_OWNER, found by tools/wsd_deal_search.py) is
// therefore a compile-time table that gives every wave a compact set of tiles with |U| <= 7 instead of a run of the
// row-major triangle: T = 13 reads 2 x 48 fragments per k-group and block where a read pair per MFMA took 2 x 169.  A wave
// keeps TWO fragment sets in registers: the MFMAs of k-group kk run from one while the reads of k-group kk + 1 fill the
// other, spread evenly between those MFMAs (sched_barriers pin the places).  All addresses are ONE base register plus
// immediates (tile index, k-group and component are compile-time), so there is still no VALU instruction between MFMAs.
// Per output tile the MFMA sequence over (chunk, k-group, h) is unchanged -- h = 0: Phi_i^T Psi_j, then h = 1: Psi_i^T Phi_j --
// so every block's partial sums are bit-identical to those of the linear deal; only the order among a wave's tiles differs
// (all h = 0 products of a k-group, then all h = 1, then the diagonal tiles: no MFMA waits for the one before it).
// Measured inside the bench (T = 13, docs/LOG_r14.md): 0.510 ms per launch against 0.529 ms with a read pair per MFMA.
// ---------------------------------------------------------------------------------------------
constexpr int wsd_ls(int T) { return ((16 * T) & 31) == 16 ? 16 * T : 16 * T + 16; }

constexpr int WSD_TMIN = 10, WSD_TMAX = 13, WSD_NTRI = WSD_TMAX * (WSD_TMAX + 1) / 2;
constexpr int WSD_MAXTILES = 12;  // accumulator tiles per wave: 96 VGPRs
constexpr int WSD_MAXU = 7;       // tile indices per wave: two fragment sets of 4 |U| VGPRs
// owner wave of every upper-triangle tile (row-major, diagonal included), one row per T = 10 ... 13; under each row its
// triangle.  Constraints of the search: <= 12 tiles per wave, |U| <= 7, the MFMAs per k-group of the SIMDs (waves w and
// w + 4) differ by at most one and those of the two waves of a SIMD by at most two; minimised: sum of |U| over the waves
constexpr signed char WSD_OWNER[WSD_TMAX - WSD_TMIN + 1][WSD_NTRI] = {
    // T = 10: tiles 6 7 7 7 7 7 7 7, MFMAs 12 12 13 12 13 13 12 13, SIMDs 25 25 25 25, sum |U| = 37
    {7, 0, 3, 3, 2, 2, 7, 2, 0, 0, 4, 0, 1, 4, 1, 4, 2, 0, 4, 3, 3, 3, 5, 5, 7, 0, 7, 1, 3, 1, 6, 6, 6, 1, 3, 5, 4, 2, 5, 4, 2, 5, 2, 5, 1, 6, 7, 6, 7, 6, 6, 7, 5, 4, 1},
    //   7 0 3 3 2 2 7 2 0 0
    //     4 0 1 4 1 4 2 0 4
    //       3 3 3 5 5 7 0 7
    //         1 3 1 6 6 6 1
    //           3 5 4 2 5 4
    //             2 5 2 5 1
    //               6 7 6 7
    //                 6 6 7
    //                   5 4
    //                     1
    // T = 11: tiles 9 9 8 9 7 9 8 7, MFMAs 16 16 16 16 14 14 15 14, SIMDs 30 30 31 30, sum |U| = 39
    {5, 0, 6, 0, 5, 3, 6, 0, 5, 5, 3, 0, 7, 7, 4, 2, 2, 0, 4, 7, 2, 6, 7, 6, 3, 6, 3, 6, 7, 3, 1, 1, 1, 0, 0, 1, 7, 1, 5, 1, 6, 4, 4, 5, 1, 1, 2, 3, 1, 2, 3, 0, 0, 6, 2, 2, 3, 4, 7, 4, 5, 5, 4, 5, 2, 3},
    //   5 0 6 0 5 3 6 0 5 5 3
    //     0 7 7 4 2 2 0 4 7 2
    //       6 7 6 3 6 3 6 7 3
    //         1 1 1 0 0 1 7 1
    //           5 1 6 4 4 5 1
    //             1 2 3 1 2 3
    //               0 0 6 2 2
    //                 3 4 7 4
    //                   5 5 4
    //                     5 2
    //                       3
    // T = 12: tiles 9 9 11 10 10 11 9 9, MFMAs 18 17 18 19 18 19 18 17, SIMDs 36 36 36 36, sum |U| = 46
    {4, 0, 0, 4, 7, 4, 7, 0, 1, 1, 0, 1, 3, 0, 6, 6, 6, 2, 0, 3, 2, 2, 3, 2, 5, 5, 0, 5, 5, 1, 1, 2, 1, 5, 6, 4, 5, 4, 6, 5, 4, 4, 5, 7, 3, 6, 3, 7, 3, 3, 7, 7, 6, 6, 7, 0, 4, 2, 5, 3, 2, 2, 7, 5, 6, 5, 0, 4, 1, 1, 3, 1, 2, 2, 7, 2, 3, 4},
    //   4 0 0 4 7 4 7 0 1 1 0 1
    //     3 0 6 6 6 2 0 3 2 2 3
    //       2 5 5 0 5 5 1 1 2 1
    //         5 6 4 5 4 6 5 4 4
    //           5 7 3 6 3 7 3 3
    //             7 7 6 6 7 0 4
    //               2 5 3 2 2 7
    //                 5 6 5 0 4
    //                   1 1 3 1
    //                     2 2 7
    //                       2 3
    //                         4
    // T = 13: tiles 12 11 11 12 11 11 12 11, MFMAs 22 21 21 21 20 21 22 21, SIMDs 42 42 43 42, sum |U| = 48
    {0, 2, 0, 0, 1, 1, 2, 2, 6, 0, 6, 2, 6, 4, 3, 3, 4, 5, 5, 2, 3, 4, 4, 4, 2, 6, 7, 3, 7, 3, 7, 3, 0, 6, 7, 7, 0, 4, 7, 3, 7, 0, 0, 4, 0, 7, 3, 1, 3, 1, 3, 1, 4, 4, 1, 5, 5, 1, 5, 5, 5, 7, 1, 3, 2, 5, 5, 5, 2, 2, 7, 6, 1, 6, 7, 6, 3, 0, 6, 0, 6, 1, 5, 0, 1, 4, 4, 6, 2, 2, 6},
    //   0 2 0 0 1 1 2 2 6 0 6 2 6
    //     4 3 3 4 5 5 2 3 4 4 4 2
    //       6 7 3 7 3 7 3 0 6 7 7
    //         0 4 7 3 7 0 0 4 0 7
    //           3 1 3 1 3 1 4 4 1
    //             5 5 1 5 5 5 7 1
    //               3 2 5 5 5 2 2
    //                 7 6 1 6 7 6
    //                   3 0 6 0 6
    //                     1 5 0 1
    //                       4 4 6
    //                         2 2
    //                           6
};
// |U| of every wave as the search states it (static_assert below)
constexpr int WSD_NU[WSD_TMAX - WSD_TMIN + 1][VXC_WAVES] = {
    {5, 4, 5, 4, 5, 5, 4, 5}, {5, 5, 5, 5, 5, 4, 5, 5}, {6, 5, 5, 6, 6, 6, 6, 6}, {6, 6, 6, 6, 6, 6, 6, 6}};

// the deal of T tile rows, derived from WSD_OWNER[T - 10]: per wave its tiles (the NO off-diagonal ones first, then the ND
// diagonal ones), the sorted tile indices U it needs and, per tile, the slots of its row and column index in U
template <int T>
struct WsdDeal {
    int nt[VXC_WAVES], no[VXC_WAVES], nu[VXC_WAVES], nm[VXC_WAVES];  // tiles, off-diagonal tiles, |U|, MFMAs per k-group
    int ti[VXC_WAVES][WSD_NTRI], tj[VXC_WAVES][WSD_NTRI];            // tile coordinates, ti <= tj
    int si[VXC_WAVES][WSD_NTRI], sj[VXC_WAVES][WSD_NTRI];            // slots of ti and tj in u
    int u[VXC_WAVES][WSD_TMAX];
    int owned;  // tiles of the triangle whose table entry names a wave (every tile has one entry: owned exactly once)
    constexpr WsdDeal() : nt{}, no{}, nu{}, nm{}, ti{}, tj{}, si{}, sj{}, u{}, owned(0) {
        for (int pass = 0; pass < 2; pass++)  // pass 0: off-diagonal tiles, pass 1: diagonal tiles
            for (int i = 0, k = 0; i < T; i++)
                for (int j = i; j < T; j++, k++) {
                    const int w = WSD_OWNER[T - WSD_TMIN][k];
                    if (w < 0 || w >= VXC_WAVES || (i == j) != (pass == 1)) continue;
                    ti[w][nt[w]] = i;
                    tj[w][nt[w]] = j;
                    nt[w]++;
                    no[w] += i != j;
                    nm[w] += i != j ? 2 : 1;
                    owned++;
                }
        for (int w = 0; w < VXC_WAVES; w++) {
            for (int x = 0; x < T; x++) {
                bool used = false;
                for (int t = 0; t < nt[w]; t++) used = used || ti[w][t] == x || tj[w][t] == x;
                if (used) u[w][nu[w]++] = x;
            }
            for (int t = 0; t < nt[w]; t++)
                for (int s = 0; s < nu[w]; s++) {
                    if (u[w][s] == ti[w][t]) si[w][t] = s;
                    if (u[w][s] == tj[w][t]) sj[w][t] = s;
                }
        }
    }
    constexpr int max_tiles() const {
        int m = 0;
        for (int w = 0; w < VXC_WAVES; w++) m = nt[w] > m ? nt[w] : m;
        return m;
    }
    constexpr int simd_spread() const {  // waves w and w + 4 share a SIMD: largest minus smallest MFMA count per k-group
        int lo = nm[0] + nm[4], hi = lo;
        for (int q = 1; q < 4; q++) {
            const int c = nm[q] + nm[q + 4];
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        return hi - lo;
    }
    constexpr int mfmas() const {
        int m = 0;
        for (int w = 0; w < VXC_WAVES; w++) m += nm[w];
        return m;
    }
    constexpr bool nu_as_stated() const {
        for (int w = 0; w < VXC_WAVES; w++)
            if (nu[w] != WSD_NU[T - WSD_TMIN][w] || nu[w] > WSD_MAXU) return false;
        return true;
    }
};
template <int T>
struct WsdDealOf {
    static constexpr WsdDeal<T> v{};
    static_assert(v.owned == T * (T + 1) / 2, "an upper-triangle tile without an owner wave");
    static_assert(v.mfmas() == T * T, "T^2 MFMAs per k-group");
    static_assert(v.max_tiles() <= WSD_MAXTILES, "more than 12 accumulator tiles per wave");
    static_assert(v.simd_spread() <= 1, "the SIMDs' MFMA counts differ by more than one");
    static_assert(v.nu_as_stated(), "per-wave fragment count |U| is not the stated one (or above 7)");
};

// LDS byte offset (from the wave's base: lk LS + lr of the current buffer) of the fragment in slot S of wave W's set,
// component X (0: Phi, 1: Psi), k-group KK
template <int T, int W, int S, int X, int KK>
constexpr int wsd_frag_off() { return (WsdDealOf<T>::v.u[W][S] * 16 + KK * VWS_GS + X * VWS_XS) * 8; }

// one chunk of consumer wave W: f[b][2 s + X] holds fragment (slot s, component X) of the k-groups with kk % 2 == b
template <int T, int W>
struct WsdChunk {
    static constexpr int NT = WsdDealOf<T>::v.nt[W], NO = WsdDealOf<T>::v.no[W], NU = WsdDealOf<T>::v.nu[W];
    static constexpr int NM = WsdDealOf<T>::v.nm[W], NR = 2 * NU;  // MFMAs and fragment reads per k-group
    typedef double Frags[2][2 * WSD_MAXU];

    template <int KK, int R>
    static DQC_DEV void read(unsigned base, Frags &f) {
        f[KK & 1][R] = *(lds_cdouble_t *)(base + wsd_frag_off<T, W, R / 2, R % 2, KK>());
    }
    template <int KK, int... R>
    static DQC_DEV void read_all(unsigned base, Frags &f, std::integer_sequence<int, R...>) {
        (read<KK, R>(base, f), ...);
    }
    // the reads of k-group KK that go in front of MFMA M of k-group KK - 1: reads [M NR / NMR, (M + 1) NR / NMR), M < NMR.
    // The last two MFMAs of a k-group carry none: every fragment is requested at least three MFMAs before its first use
    static constexpr int NMR = NM > 2 ? NM - 2 : 1;
    template <int KK, int M, int R = M * NR / NMR>
    static DQC_DEV void read_slice(unsigned base, Frags &f) {
        if constexpr (M < NMR && R < (M + 1) * NR / NMR) {
            read<KK, R>(base, f);
            read_slice<KK, M, R + 1>(base, f);
        }
    }
    // MFMA M of k-group KK: M < NO: tile M, h = 0 (Phi_i^T Psi_j); M < 2 NO: tile M - NO, h = 1 (Psi_i^T Phi_j); then the
    // diagonal tiles (Phi_i^T Psi_i)
    template <int KK, int M>
    static DQC_DEV void step(unsigned base, Frags &f, v4d (&acc)[NT]) {
        constexpr int t = M < NO ? M : M - NO, h = M >= NO && M < 2 * NO ? 1 : 0;
        constexpr int a = 2 * WsdDealOf<T>::v.si[W][t] + h, b = 2 * WsdDealOf<T>::v.sj[W][t] + (1 - h);
        if constexpr (KK < 3) read_slice<KK + 1, M>(base, f);
        __builtin_amdgcn_sched_barrier(0);
        acc[t] = mfma_f64(f[KK & 1][a], f[KK & 1][b], acc[t]);
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int KK, int... M>
    static DQC_DEV void kgroup(unsigned base, Frags &f, v4d (&acc)[NT], std::integer_sequence<int, M...>) {
        (step<KK, M>(base, f, acc), ...);
    }
    static DQC_DEV void run(unsigned base, v4d (&acc)[NT]) {
        Frags f;
        read_all<0>(base, f, std::make_integer_sequence<int, NR>{});
        kgroup<0>(base, f, acc, std::make_integer_sequence<int, NM>{});
        kgroup<1>(base, f, acc, std::make_integer_sequence<int, NM>{});
        kgroup<2>(base, f, acc, std::make_integer_sequence<int, NM>{});
        kgroup<3>(base, f, acc, std::make_integer_sequence<int, NM>{});
    }
    // off-diagonal tiles hold 2 V_ij (symmetrize_kernel halves them against the zero lower tiles), diagonal tiles M_ii
    template <int... TL>
    static DQC_DEV void store(double *__restrict__ vmat, const v4d (&acc)[NT], int lr, int lk, std::integer_sequence<int, TL...>) {
        auto one = [&](int t, int ti, int tj) {
            const int ia = ti * 16 + lk, ib = tj * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; r++) acc_add(&vmat[(size_t)(ia + 4 * r) * (16 * T) + ib], acc[t][r], g_vxc_det_scale);
        };
        (one(TL, WsdDealOf<T>::v.ti[W][TL], WsdDealOf<T>::v.tj[W][TL]), ...);
    }
};

template <int T, int W>
DQC_DEV void wsd_consumer(double *lds, double *__restrict__ vmat, int nchunk) {
    typedef WsdChunk<T, W> CH;
    constexpr int LS = wsd_ls(T);  // rows of the output matrix: 16 T; LDS rows: == 16 (mod 32)
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    v4d acc[CH::NT];
#pragma unroll
    for (int t = 0; t < CH::NT; t++) acc[t] = v4d{0, 0, 0, 0};
    // LDS byte address of tile index 0's fragment in the Phi part (k-group 0, current buffer)
    unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds + 8u * (unsigned)(lk * LS + lr);
    __syncthreads();
    for (int c = 0; c < nchunk; c++) {
        __syncthreads();  // chunk c - 1 done: the producers' combine window opens ...
        __syncthreads();  // ... and closes
        CH::run(base, acc);
        base += (c & 1) ? (unsigned)(-VWS_BUF * 8) : (unsigned)(VWS_BUF * 8);
    }
    CH::store(vmat, acc, lr, lk, std::make_integer_sequence<int, CH::NT>{});
}

template <int T, int NLP>
__global__ __launch_bounds__(VWU_NT, 3) void vxc_wsd_kernel(double *__restrict__ vmat, const double *__restrict__ ao, int ngrid,
                                                           const double *__restrict__ w, const double *__restrict__ vrho,
                                                           const double *__restrict__ vgrad, int slab, int lda) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int KCH = 16, ld = 16 * T;
    static_assert(T >= WSD_TMIN && T <= WSD_TMAX, "no ownership table for this T");
    const int wave = threadIdx.x >> 6;
    const int gs = blockIdx.x * slab, ge = min(gs + slab, ngrid);
    if (gs >= ngrid) return;
    const int nchunk = (ge - gs + KCH - 1) / KCH;
    if (wave >= VXC_WAVES) {
        vwu_producer<NLP, true>(lds, ao, ngrid, ld, w, vrho, vgrad, gs, ge, nchunk, lda, wsd_ls(T));
        return;
    }
#define DQC_WSD_CASE(W) case W: wsd_consumer<T, W>(lds, vmat, nchunk); break;
    switch (wave) {  // wave-uniform; every wave has its own straight-line body (its tile indices are immediates)
        DQC_WSD_CASE(0) DQC_WSD_CASE(1) DQC_WSD_CASE(2) DQC_WSD_CASE(3)
        DQC_WSD_CASE(4) DQC_WSD_CASE(5) DQC_WSD_CASE(6) DQC_WSD_CASE(7)
    }
#undef DQC_WSD_CASE
}

// V = (M + M^T) / 2 on the (ld, ld) matrix (deterministic mode: M arrives as fixed-point integers).  Rows / columns nao .. ld - 1
// are ZEROED: the kernels stage 16 T columns per AO row, and where the row stride of the AO arrays is below that
// (dqc_ao_stride) the last tile's extra columns hold the first values of the next row -- finite numbers that only reach
// these padding rows / columns
__global__ void symmetrize_kernel(double *m, int ld, int nao) {
    const int i = blockIdx.y * 16 + threadIdx.y, j = blockIdx.x * 16 + threadIdx.x;
    const double sc = g_vxc_det_scale;
    if (i < ld && j < i) {
        const double v = i < nao ? 0.5 * (det_value(m[(size_t)i * ld + j], sc) + det_value(m[(size_t)j * ld + i], sc)) : 0.0;
        m[(size_t)i * ld + j] = v;
        m[(size_t)j * ld + i] = v;
    } else if (i < ld && j == i) {
        if (i >= nao) m[(size_t)i * ld + i] = 0.0;
        else if (sc != 0.0) m[(size_t)i * ld + i] = det_value(m[(size_t)i * ld + i], sc);
    }
}

// deterministic mode (dqc_set_deterministic): the device-side scale follows the host flag, per device
static int sync_vxc_det_scale() {
    static double current[64];  // what each device's g_vxc_det_scale holds (0: fp64 atomics)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    // |V_ij| <= max |v_xc| int |phi_i phi_j| stays far below 2^14 for normalised AOs: 2^47 leaves the sum 63 bits
    const double want = deterministic_mode() ? 140737488355328.0 : 0.0;
    if (current[dev] != want) {
        DQC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_vxc_det_scale), &want, sizeof(double)));
        current[dev] = want;
    }
    return 0;
}

template <int MAXT, int NLP, int KCH, bool GGA>
static void launch_vxc_ws_inst(dim3 grid, size_t shmem, hipStream_t st, double *vmat, const double *ao, int ngrid, int ld,
                               const double *w, const double *vrho, const double *vgrad, int slab, int nsplit, int tps,
                               const double *aob, int sym, int lda, int LS) {
    auto kern = vxc_ws_kernel<MAXT, NLP, KCH, GGA>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL(kern, grid, dim3(VWS_NT), shmem, st, vmat, ao, ngrid, ld, w, vrho, vgrad, slab, nsplit, tps, aob, sym, lda, LS);
}

template <bool GGA>
static int launch_vxc_ws(int maxt, int nlp, dim3 grid, size_t shmem, hipStream_t st, double *vmat,
                         const double *ao, int ngrid, int ld, const double *w, const double *vrho, const double *vgrad,
                         int slab, int nsplit, int tps, const double *aob, int sym, int lda, int LS) {
#define DQC_VWS_CASE(N, L)                                                                                          \
    if (maxt == N && nlp == L) {                                                                                    \
        launch_vxc_ws_inst<N, L, 16, GGA>(grid, shmem, st, vmat, ao, ngrid, ld, w, vrho, vgrad, slab, nsplit, tps, aob, sym, lda, LS); \
        return 0;                                                                                                   \
    }
    DQC_VWS_CASE(2, 1) DQC_VWS_CASE(4, 1) DQC_VWS_CASE(6, 1) DQC_VWS_CASE(8, 1) DQC_VWS_CASE(11, 1)
    DQC_VWS_CASE(2, 2) DQC_VWS_CASE(4, 2) DQC_VWS_CASE(6, 2) DQC_VWS_CASE(8, 2) DQC_VWS_CASE(11, 2)
    DQC_VWS_CASE(2, 4) DQC_VWS_CASE(4, 4) DQC_VWS_CASE(6, 4) DQC_VWS_CASE(8, 4) DQC_VWS_CASE(11, 4)
#undef DQC_VWS_CASE  // (ld <= 256 with 32 producer threads per row needs at most 4 pieces per thread)
    set_error("vxc_ws: internal dispatch error");
    return DQC_EINVAL;
}

template <int MAXT>
static void launch_vxc_wsu(dim3 grid, size_t shmem, hipStream_t st, double *vmat, const double *ao, int ngrid, int ld,
                                const double *w, const double *vrho, const double *vgrad, int slab, int lda, int LS) {
    auto kern = vxc_wsu_kernel<MAXT, 7>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL(kern, grid, dim3(VWU_NT), shmem, st, vmat, ao, ngrid, ld, w, vrho, vgrad, slab, lda, LS);
}

template <int T>
static void launch_vxc_wsd(dim3 grid, size_t shmem, hipStream_t st, double *vmat, const double *ao, int ngrid, const double *w,
                           const double *vrho, const double *vgrad, int slab, int lda) {
    auto kern = vxc_wsd_kernel<T, 7>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL(kern, grid, dim3(VWU_NT), shmem, st, vmat, ao, ngrid, w, vrho, vgrad, slab, lda);
}

template <int MAXT, int NLA, int NLB, bool GGA>
static void launch_vxc_ws2_inst(dim3 grid, size_t shmem, hipStream_t st, double *vmat, const double *ao, int ngrid, int ld,
                                const double *w, const double *vrho, const double *vgrad, int slab, int NR, int NC, int LSA,
                                int LSB, const double *aob, int lda) {
    auto kern = vxc_ws2_kernel<MAXT, NLA, NLB, GGA>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL(kern, grid, dim3(VWS2_NT), shmem, st, vmat, ao, ngrid, ld, w, vrho, vgrad, slab, NR, NC, LSA, LSB, aob, lda);
}

template <bool GGA>
static int launch_vxc_ws2(int maxt, int nla, int nlb, dim3 grid, size_t shmem, hipStream_t st, double *vmat, const double *ao,
                          int ngrid, int ld, const double *w, const double *vrho, const double *vgrad, int slab, int NR,
                          int NC, int LSA, int LSB, const double *aob, int lda) {
#define DQC_VW2_CASE(N, A, B)                                                                                        \
    if (maxt == N && nla == A && nlb == B) {                                                                          \
        launch_vxc_ws2_inst<N, A, B, GGA>(grid, shmem, st, vmat, ao, ngrid, ld, w, vrho, vgrad, slab, NR, NC, LSA, LSB, aob, lda); \
        return 0;                                                                                                     \
    }
    DQC_VW2_CASE(8, 4, 4) DQC_VW2_CASE(8, 4, 6) DQC_VW2_CASE(11, 4, 4) DQC_VW2_CASE(11, 4, 6)
    DQC_VW2_CASE(8, 5, 4) DQC_VW2_CASE(8, 5, 6) DQC_VW2_CASE(11, 5, 4) DQC_VW2_CASE(11, 5, 6)  // 9-row rectangles (NLA = 5)
#undef DQC_VW2_CASE
    set_error("vxc_ws2: internal dispatch error");
    return DQC_EINVAL;
}

}  // namespace dqc

extern "C" {

static int grid_vxc_impl(double *d_vmat, const double *d_ao, const double *d_aob, int ncomp, int ngrid, int nao,
                         const double *d_w, const double *d_vrho, const double *d_vgrad, void *stream, bool raw = false) {
    // raw: the cross-block sums M are left as the kernels wrote them (V = (M + M^T) / 2 restricted to the first nao rows / columns is
    // formed by the consumer: dqc_fock_finish with vxc_raw) -- one launch less per build
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    const bool gga = d_vgrad != nullptr;
    if (gga && ncomp < 4) { set_error("dqc_grid_vxc: vgrad given but ao has < 4 components"); return DQC_EINVAL; }
    // ld, lda, LS: see the head of the file
    const int ld = dqc_padded_nao(nao), lda = dqc_ao_stride(nao), T = ld / 16;
    auto pad16 = [](int w_) { return (w_ & 31) == 16 ? w_ : w_ + 16; };
    const int LS = pad16(ld);
    if (sync_vxc_det_scale()) return DQC_EHIP;
    DQC_HIP(hipMemsetAsync(d_vmat, 0, sizeof(double) * (size_t)ld * ld, st));
    if (ngrid <= 0) return DQC_OK;
    // ws_shape: a whole staged row fits the fixed-stride chunk layout of vxc_ws / vxc_wsu / vxc_wsd (T <= 15)
    const bool ws_shape = LS <= VWS_LSMAX, one_operand = d_aob == d_ao;
    // one-operand forms without a gradient term (LDA Vxc, the tau terms of a meta-GGA) are symmetric matrices: vxc_ws_kernel
    // then computes the upper-triangular tiles only
    const bool sym = ws_shape && !gga && one_operand;
    const int ttot = sym ? T * (T + 1) / 2 : T * T;  // tiles to compute
    auto slabs = [&](int nslab, int mult, int &slab) {  // `nslab` slabs of a multiple of 16 points; -> slab count, a multiple of `mult`
        slab = (ngrid + nslab - 1) / nslab;
        slab = (slab + 15) / 16 * 16;
        return ((ngrid + slab - 1) / slab + mult - 1) / mult * mult;
    };
    int rc = 0, slab = 0;
    if (ttot > 2 * 11 * VXC_WAVES) {
        // ---- vxc_ws2_kernel (larger bases): rectangular ownership, rectangles of at most 9 x 12 tiles.
        // Rectangle shape: a block stages nr Phi tile columns (one component) and 4 nc AO-component tile columns for its
        // nr x nc tiles -- (nr + 4 nc) / (nr nc) operand tile columns per MFMA: rows are cheap, columns dear.  The tallest
        // rectangle the layout allows (9 rows: LSA <= 144), then the widest that keeps <= 11 accumulator tiles per wave:
        // T = 26 (naphthalene / cc-pVTZ): 9 x 9 tiles, 9 blocks per slab (round 2: 7 x 9, 12 blocks); T = 17: 9 x 9 (6 x 9).
        // DQC_WS2_NR / DQC_WS2_NC override the block counts (A/B runs).
        int NR = (T + 8) / 9, NC = 1;
        {
            const int nrm = (T + NR - 1) / NR;
            while ((T + NC - 1) / NC > 12 || nrm * ((T + NC - 1) / NC) > 11 * VXC_WAVES) NC++;
            const char *e1 = getenv("DQC_WS2_NR"), *e2 = getenv("DQC_WS2_NC");
            if (e1 && atoi(e1) > 0) NR = atoi(e1);
            if (e2 && atoi(e2) > 0) NC = atoi(e2);
        }
        const int nrmax = (T + NR - 1) / NR, ncmax = (T + NC - 1) / NC;
        if (nrmax > 9 || ncmax > 12 || nrmax * ncmax > 11 * VXC_WAVES) { set_error("vxc_ws2: rectangle outside the kernel's limits"); return DQC_EINVAL; }
        const int need = (nrmax * ncmax + VXC_WAVES - 1) / VXC_WAVES;
        const int maxt = need <= 8 ? 8 : 11;
        const int LSA = pad16(nrmax * 16), LSB = pad16(ncmax * 16);
        if (LSA > 144 || LSB > 208) { set_error("vxc_ws2: internal layout error"); return DQC_EINVAL; }
        const int nla = nrmax <= 8 ? 4 : 5, nlb = (ncmax * 8 + 15) / 16 <= 4 ? 4 : 6;  // b128 loads per producer thread and row
        const int nsplit = NR * NC;
        // two blocks per CU: the nine (NR x NC) blocks of a slab start together and stay in step (see the consumers), so the slab
        // is fetched from HBM about once; many small blocks (DQC_VXC_BLOCKS=3072: ~12 per CU) even out the tail but start
        // at different times -- same launch time, FETCH_SIZE x 2 (profiles/r04q_c4_blocks.txt)
        static const int target_blocks = [] { const char *e = getenv("DQC_VXC_BLOCKS"); return e && atoi(e) > 0 ? atoi(e) : 512; }();
        // slabs in multiples of 8 so that the XCD-aware decode is exact
        const int nslab = slabs(std::max(8, std::min(target_blocks / nsplit, std::max(ngrid / 1024, 512 / nsplit)) / 8 * 8), 8, slab);
        const size_t shmem = sizeof(double) * 2 * WS2_BUF;  // fixed-stride chunk layout, two buffers
        const dim3 grid(nslab * nsplit);
        rc = gga ? launch_vxc_ws2<true>(maxt, nla, nlb, grid, shmem, st, d_vmat, d_ao, ngrid, ld, d_w, d_vrho, d_vgrad, slab, NR, NC, LSA, LSB, d_aob, lda)
                 : launch_vxc_ws2<false>(maxt, nla, nlb, grid, shmem, st, d_vmat, d_ao, ngrid, ld, d_w, d_vrho, d_vgrad, slab, NR, NC, LSA, LSB, d_aob, lda);
    } else if (ws_shape && T >= 10 && T * (T + 1) / 2 <= 12 * VXC_WAVES && one_operand) {
        // ---- vxc_wsu_kernel / vxc_wsd_kernel: 145 <= nao <= 208 (10 <= T <= 13), one operand: one block per slab over the
        // upper-triangular tiles instead of two blocks that each stage the whole slab
        int ncu = stream_cus(st);  // one block per CU of the stream's partition (all 256 on an ordinary stream)
        if (vxc_cus_cap() > 0) ncu = std::max(8, std::min(ncu, vxc_cus_cap()));  // (leave CUs to other streams' kernels: host.hip)
        const dim3 grid(slabs(ncu, 1, slab));
        const size_t shmem = sizeof(double) * 2 * VWS_BUF;
        if (gga) {  // one MFMA on the diagonal tiles, two on the others
            if (T == 13) launch_vxc_wsd<13>(grid, shmem, st, d_vmat, d_ao, ngrid, d_w, d_vrho, d_vgrad, slab, lda);
            else if (T == 12) launch_vxc_wsd<12>(grid, shmem, st, d_vmat, d_ao, ngrid, d_w, d_vrho, d_vgrad, slab, lda);
            else if (T == 11) launch_vxc_wsd<11>(grid, shmem, st, d_vmat, d_ao, ngrid, d_w, d_vrho, d_vgrad, slab, lda);
            else launch_vxc_wsd<10>(grid, shmem, st, d_vmat, d_ao, ngrid, d_w, d_vrho, d_vgrad, slab, lda);
        } else if ((T * (T + 1) / 2 + VXC_WAVES - 1) / VXC_WAVES <= 9) {  // accumulator tiles per wave
            launch_vxc_wsu<9>(grid, shmem, st, d_vmat, d_ao, ngrid, ld, d_w, d_vrho, d_vgrad, slab, lda, LS);
        } else {
            launch_vxc_wsu<12>(grid, shmem, st, d_vmat, d_ao, ngrid, ld, d_w, d_vrho, d_vgrad, slab, lda, LS);
        }
    } else if (ws_shape) {
        // ---- vxc_ws_kernel (8 MFMA waves + 8 producer waves): the tiles are split linearly over 1 or 2 blocks per slab; tiles
        // per block are capped at 11 per wave so that accumulators + prefetch registers fit 256 VGPRs
        static const int sizes_ws[] = {2, 4, 6, 8, 11};
        const int cap = 11 * VXC_WAVES;
        const int nsplit = (ttot + cap - 1) / cap;
        const int tps = (ttot + nsplit - 1) / nsplit;
        const int need = (tps + VXC_WAVES - 1) / VXC_WAVES;
        int maxt = 11;
        for (int q = 0; q < 5; q++)
            if (sizes_ws[q] >= need) { maxt = sizes_ws[q]; break; }
        // the producers hold a whole chunk in registers: b128 pieces per thread and row (ws_shape: ld <= 240, at most 4)
        const int tprp = VWS_PROD / 16;
        const int nlpneed = (ld / 2 + tprp - 1) / tprp;
        const int nlp = nlpneed <= 1 ? 1 : (nlpneed <= 2 ? 2 : 4);
        // one block per CU; slabs in multiples of 8 so that the XCD-aware decode is exact
        const int nslab = slabs(std::max(8, (stream_cus(st) / nsplit) / 8 * 8), 8, slab);
        const size_t shmem = sizeof(double) * 2 * VWS_BUF;  // fixed-stride chunk layout, two buffers
        const dim3 grid(nslab * nsplit);
        rc = gga ? launch_vxc_ws<true>(maxt, nlp, grid, shmem, st, d_vmat, d_ao, ngrid, ld, d_w, d_vrho, d_vgrad, slab, nsplit, tps, d_aob, 0, lda, LS)
                 : launch_vxc_ws<false>(maxt, nlp, grid, shmem, st, d_vmat, d_ao, ngrid, ld, d_w, d_vrho, d_vgrad, slab, nsplit, tps, d_aob, sym ? 1 : 0, lda, LS);
    } else {
        // (not reached: without ws_shape T >= 16 and ttot = T^2 takes the first branch)
        set_error("dqc_grid_vxc: internal dispatch error (no kernel family for this shape)");
        return DQC_EINVAL;
    }
    if (rc) return rc;
    DQC_CHECK_LAUNCH();
    if (!raw) hipLaunchKernelGGL(symmetrize_kernel, dim3((ld + 15) / 16, (ld + 15) / 16), dim3(16, 16), 0, st, d_vmat, ld, nao);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

int dqc_grid_vxc(double *d_vmat, const double *d_ao, int ncomp, int ngrid, int nao, const double *d_w,
                 const double *d_vrho, const double *d_vgrad, void *stream) {
    return grid_vxc_impl(d_vmat, d_ao, d_ao, ncomp, ngrid, nao, d_w, d_vrho, d_vgrad, stream);
}

int dqc_grid_vxc_raw(double *d_vmat, const double *d_ao, int ncomp, int ngrid, int nao, const double *d_w, const double *d_vrho,
                     const double *d_vgrad, double *h_scale, void *stream) {
    // dqc_grid_vxc without its closing symmetrisation launch: d_vmat <- the raw cross-block sums M (fixed-point integers in
    // deterministic mode; *h_scale <- their scale, 0: plain doubles), V = (M + M^T) / 2 on the first nao rows / columns
    if (h_scale) *h_scale = dqc::deterministic_mode() ? 140737488355328.0 : 0.0;
    return grid_vxc_impl(d_vmat, d_ao, d_ao, ncomp, ngrid, nao, d_w, d_vrho, d_vgrad, stream, true);
}

int dqc_grid_vxc_pair(double *d_vmat, const double *d_ao_a, const double *d_ao_b, int ngrid, int nao, const double *d_w,
                      const double *d_v, void *stream) {
    return grid_vxc_impl(d_vmat, d_ao_a, d_ao_b, 1, ngrid, nao, d_w, d_v, nullptr, stream);
}

#ifdef VWU_TRACE
int dqc_debug_vwu_trace(long long *host_out) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(dqc::g_vwu_trace), sizeof(long long) * 2 * dqc::VWU_TRACE_N);
}
#endif


}  // extern "C"
