// mp2.hip -- RI-MP2 pair energies from the occupied-virtual three-index tensors, fused: the (ia|jb) never leave the registers.
//
//     V^{ij}_{ab} = sum_P Bi[i, P, a] Bj[j, P, b]  ( = (ia|jb) ),     D^{ij}_{ab} = eps_i + eps_j - eps_a - eps_b
//     e_os[i, j] = sum_ab V_ab^2 / D_ab,     e_ss[i, j] = sum_ab V_ab (V_ab - V_ba) / D_ab      (e_ss: same mode only)
//
// Bi[i, P, a]: one (naux, ldv) slab per occupied orbital, ldv the virtual count padded to a multiple of 16.
//
// One block (four waves) owns one occupied pair (i, j) and one 64 x 64 panel pair (Ap, Bp) of the virtual space -- 4 x 4 tiles of
// 16 x 16; wave w owns tile row A = 4 Ap + w and the four tiles B = 4 Bp + t of it.  The panels Bi[:, Ap], Bj[:, Bp] (and, same mode,
// Bj[:, Ap], Bi[:, Bp]) are staged in LDS in chunks of MP2_KC auxiliary functions -- each element is read from memory once per block
// and from LDS by four (A panels: one) waves; the next chunk is asked for before the MFMAs of this one and stored after them (mp2_sweep,
// which every kernel of this file calls).  LDS row stride 80 doubles (== 32 banks mod 64): the two k rows a 32-lane half reads with
// ds_read_b64 sit 32 banks apart, conflict-free.
//
// Same mode (restricted, alpha-alpha, beta-beta: Bi == Bj as tensors): only i <= j, only panel pairs Ap <= Bp and in a diagonal panel pair
// only tiles A <= B.  Per tile pair two accumulators with v_mfma_f64_16x16x4_f64:
//     acc1 = Bi[:, A]^T Bj[:, B]            -> C[row a][col b] = V_ab
//     acc2 = Bj[:, A]^T Bi[:, B]            -> C[row a][col b] = sum_P Bj[j, P, a] Bi[i, P, b] = (ib|ja) = V_ba
// i.e. the second tile is formed already transposed: V_ba lands in the lane and register of V_ab (C/D map col = lane & 15,
// row = (lane >> 4) + 4 reg) and the epilogue needs no shuffle and no LDS transpose.  D_ab = D_ba, so an off-diagonal tile pair
// contributes V_ab^2 + V_ba^2 to e_os and (V_ab - V_ba)^2 to e_ss; a diagonal one V_ab^2 and V_ab (V_ab - V_ba).
// Opposite mode (alpha-beta): rectangular, every (i, j), every tile, one accumulator, e_os only.
//
// Padded virtuals (a >= nva or b >= nvb) are masked in the epilogue (their denominator is replaced by 1, their term by 0): whatever the
// padding columns hold, they contribute exactly zero.  The partial sums of a block -- lanes by butterfly, waves in order -- go to its slot
// of the work buffer, and mp2_sum_kernel adds the slots of a pair in slot order: no atomics, bit-reproducible as it stands.
//
// Amplitudes (mp2_amp_kernel, dqc_mp2_amplitudes): the same staging and the same two accumulators, same mode only, for the occupied
// block i in [i0, i0 + ni) against every j -- ordered pairs, one block per (i, j, panel pair Ap <= Bp) -- but the epilogue STORES
//     T[i - i0, j, a, b] = V_ab / D_ab,       Tt[i - i0, j, a, b] = (c_os + c_ss) T_ab - c_ss T_ba        (two (ni, noj, ldv, ldv) buffers)
// THE CHOICE FOR THE LOWER TRIANGLE: tiles B < A are not computed.  acc2 of the tile pair A < B IS the tile (B, A) of V, held
// transposed (V_ba in the lane of V_ab), so the wave stores (a, b) straight from its registers and (b, a) through a 16 x 17 LDS
// scratch of its own: written [b][a], read back by rows.  Every store instruction of a wave is then four full 128-byte rows (the 16
// lanes of equal lane >> 4 write 16 consecutive b), each V element costs one MFMA pass (2 naux flop), and T^{ij}_{ab}, T^{ji}_{ba}
// are bit-equal: the same products in the same order, and D is formed as (eps_i + eps_j) - (eps_a + eps_b), symmetric term by term.
// The (ldv, ldv) faces are written whole: a >= nv or b >= nv is stored as 0.0 whatever the inputs' padding columns hold (tiles that
// hold no real virtual skip their MFMAs).  Every element is written once, by one lane: no atomics, bit-reproducible.
#include "common.hpp"
#include "mfma_tile.hpp"

namespace dqc {

constexpr int MP2_KC = 16;   // auxiliary functions per LDS chunk
constexpr int MP2_PW = 64;   // panel width (four tiles)
constexpr int MP2_LS = 80;   // LDS row stride in doubles

struct Mp2Args {
    const double *bi, *bj, *eoi, *eoj, *eva, *evb;
    double *part;  // [pair][panel pair][2]
    int noi, noj, nva, nvb, ldva, ldvb, naux;
    int npa, npb;        // panels of 64 per side
    long long ntp;       // panel pairs per occupied pair
};

// two consecutive doubles of row k of a panel (zero past naux and past ld)
DQC_DEV double2 mp2_load2(const double *slab, int ld, int naux, int k, int col) {
    if (k < naux && col < ld) return *reinterpret_cast<const double2 *>(slab + (size_t)k * ld + col);
    return double2{0.0, 0.0};
}

// The sweep over the auxiliary index of one block, the one copy of it: NP panels of 64 columns (panel p: columns scol[p] ... of the
// slab src[p] of row length sld[p]), [Bi A][Bj B] and, NP == 4, [Bj A][Bi B], staged in chunks of MP2_KC rows -- 16 rows x 32 double2
// per panel = 512 double2, two per thread and panel; the next chunk is asked for before the MFMAs of this one and stored after them,
// two barriers per chunk.  On return acc1[t] (and, NP == 4, acc2[t]) hold the tiles live[t] of wave `wave`; the others are zero.
// g: the kernel's argument block, of which naux is read (handed on whole, as the kernels read it before the sweep was shared: with
// naux as a value of the caller the compiler lays mp2_pair_kernel<true> out four bytes shorter in front of the chunk loop, which costs
// 1.3 % there -- docs/LOG_r25.md).
template <int NP, class Args>
DQC_DEV void mp2_sweep(double (&s_p)[NP][MP2_KC][MP2_LS], const double *const (&src)[NP], const int (&sld)[NP], const int (&scol)[NP],
                       const Args &g, int wave, int l15, int q, const bool (&live)[4], v4d (&acc1)[4], v4d (&acc2)[4]) {
    const int naux = g.naux;
    const bool any = live[0] || live[1] || live[2] || live[3];
#pragma unroll
    for (int t = 0; t < 4; t++) acc1[t] = acc2[t] = v4d{0.0, 0.0, 0.0, 0.0};

    double2 nx[NP][2];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = threadIdx.x + 256 * u, k = e >> 5, c2 = (e & 31) * 2;
                nx[p][u] = mp2_load2(src[p], sld[p], naux, c0 + k, scol[p] + c2);
            }
    };
    fetch(0);
    for (int c0 = 0; c0 < naux; c0 += MP2_KC) {
        __syncthreads();  // (the previous chunk has been read by every wave)
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = threadIdx.x + 256 * u, k = e >> 5, c2 = (e & 31) * 2;
                *reinterpret_cast<double2 *>(&s_p[p][k][c2]) = nx[p][u];
            }
        __syncthreads();
        if (c0 + MP2_KC < naux) fetch(c0 + MP2_KC);
        if (!any) continue;
        const int nk = min(MP2_KC, (naux - c0 + 3) & ~3);  // (rows past naux are zero: whole k-steps of them are skipped)
        for (int k0 = 0; k0 < nk; k0 += 4) {
            const double ai = s_p[0][k0 + q][16 * wave + l15];
            double aj = 0.0;
            if constexpr (NP == 4) aj = s_p[2][k0 + q][16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (!live[t]) continue;  // (wave-uniform)
                acc1[t] = mfma_f64(ai, s_p[1][k0 + q][16 * t + l15], acc1[t]);
                if constexpr (NP == 4) acc2[t] = mfma_f64(aj, s_p[3][k0 + q][16 * t + l15], acc2[t]);
            }
        }
    }
}

// the rows of a lane in tile row tA, a = 16 tA + q + 4 r: inside the virtual space? and their orbital energies (0.0 outside)
DQC_DEV void mp2_rows(const double *ev, int nv, int tA, int q, double (&ea)[4], bool (&oka)[4]) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a = 16 * tA + q + 4 * r;
        oka[r] = a < nv;
        ea[r] = oka[r] ? ev[a] : 0.0;
    }
}

template <bool SAME>
__global__ __launch_bounds__(256, 2) void mp2_pair_kernel(Mp2Args g) {
    constexpr int NP = SAME ? 4 : 2;  // staged panels: [Bi A][Bj B] ([Bj A][Bi B])
    __shared__ __align__(16) double s_p[NP][MP2_KC][MP2_LS];
    __shared__ double s_red[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    const long long pair = blockIdx.x / g.ntp, tp = blockIdx.x - pair * g.ntp;
    int i, j, pa, pb;
    if (SAME) {
        tri_index(pair, i, j);
        tri_index(tp, pa, pb);
    } else {
        i = (int)(pair / g.noj);
        j = (int)(pair - (long long)i * g.noj);
        pa = (int)(tp / g.npb);
        pb = (int)(tp - (long long)pa * g.npb);
    }
    const double *slab_i = g.bi + (size_t)i * g.naux * g.ldva, *slab_j = g.bj + (size_t)j * g.naux * g.ldvb;
    const double *src[NP];
    int sld[NP], scol[NP];
    src[0] = slab_i; sld[0] = g.ldva; scol[0] = pa * MP2_PW;
    src[1] = slab_j; sld[1] = g.ldvb; scol[1] = pb * MP2_PW;
    if constexpr (SAME) {
        src[2] = slab_j; sld[2] = g.ldvb; scol[2] = pa * MP2_PW;
        src[3] = slab_i; sld[3] = g.ldva; scol[3] = pb * MP2_PW;
    }
    const int tA = 4 * pa + wave;  // this wave's tile row
    // tiles this wave forms: those that hold a real virtual on both sides (and, same mode, A <= B)
    bool live[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int tB = 4 * pb + t;
        live[t] = 16 * tA < g.nva && 16 * tB < g.nvb && (!SAME || tA <= tB);
    }
    const bool any = live[0] || live[1] || live[2] || live[3];
    v4d acc1[4], acc2[4];
    mp2_sweep<NP>(s_p, src, sld, scol, g, wave, l15, q, live, acc1, acc2);
    // epilogue: lane (l15, q), register r holds a = 16 tA + q + 4 r, b = 16 tB + l15
    double eos = 0.0, ess = 0.0;
    if (any) {
        const double eij = g.eoi[i] + g.eoj[j];
        double ea[4];
        bool oka[4];
        mp2_rows(g.eva, g.nva, tA, q, ea, oka);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (!live[t]) continue;
            const int tB = 4 * pb + t, b = 16 * tB + l15;
            const bool okb = b < g.nvb;
            const double eb = okb ? g.evb[b] : 0.0;
            const bool offdiag = SAME && tA != tB;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool ok = oka[r] && okb;
                const double d = ok ? eij - ea[r] - eb : 1.0;
                const double v = ok ? acc1[t][r] : 0.0;
                if (SAME) {
                    const double vt = ok ? acc2[t][r] : 0.0, df = v - vt;
                    eos += (offdiag ? v * v + vt * vt : v * v) / d;
                    ess += (offdiag ? df * df : v * df) / d;
                } else {
                    eos += v * v / d;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        eos += __shfl_xor(eos, o);
        ess += __shfl_xor(ess, o);
    }
    if (lane == 0) { s_red[wave][0] = eos; s_red[wave][1] = ess; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *out = g.part + 2 * (size_t)blockIdx.x;
        out[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
        out[1] = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
    }
}

// the slots of a pair in slot order; same mode: mirrored into [j][i]
__global__ __launch_bounds__(64) void mp2_sum_kernel(double *__restrict__ eos, double *__restrict__ ess, const double *__restrict__ part,
                                                     long long npair, long long ntp, int noj, int same) {
    const long long pair = (long long)blockIdx.x * 64 + threadIdx.x;
    if (pair >= npair) return;
    double a = 0.0, b = 0.0;
    for (long long s = 0; s < ntp; s++) {
        a += part[2 * (pair * ntp + s)];
        b += part[2 * (pair * ntp + s) + 1];
    }
    if (same) {
        int i, j;
        tri_index(pair, i, j);
        eos[(size_t)i * noj + j] = a;
        eos[(size_t)j * noj + i] = a;
        ess[(size_t)i * noj + j] = b;
        ess[(size_t)j * noj + i] = b;
    } else {
        eos[pair] = a;
    }
}

struct Mp2AmpArgs {
    const double *b, *eo, *ev;
    double *t, *tt;      // [i - i0][j][a][b], faces of ldv x ldv
    double c1, c2;       // Tt = c1 T - c2 T^T: c_os + c_ss, c_ss
    int noj, nv, ldv, naux, i0;
    long long ntp;       // panel pairs per occupied pair
};

__global__ __launch_bounds__(256, 2) void mp2_amp_kernel(Mp2AmpArgs g) {
    __shared__ __align__(16) double s_p[4][MP2_KC][MP2_LS];  // [Bi A][Bj B][Bj A][Bi B]
    __shared__ double s_tr[4][16][17];                       // per wave: one tile on its way to the transposed position
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    const long long pair = blockIdx.x / g.ntp, tp = blockIdx.x - pair * g.ntp;  // pair = (i - i0) noj + j
    const int il = (int)(pair / g.noj), j = (int)(pair - (long long)il * g.noj), i = g.i0 + il;
    int pa, pb;
    tri_index(tp, pa, pb);
    const double *slab_i = g.b + (size_t)i * g.naux * g.ldv, *slab_j = g.b + (size_t)j * g.naux * g.ldv;
    const double *src[4] = {slab_i, slab_j, slab_j, slab_i};
    const int sld[4] = {g.ldv, g.ldv, g.ldv, g.ldv};
    const int scol[4] = {pa * MP2_PW, pb * MP2_PW, pa * MP2_PW, pb * MP2_PW};
    const int tA = 4 * pa + wave;
    bool inside[4], live[4];  // the tile pair is this wave's to store; it holds a real virtual on both sides
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int tB = 4 * pb + t;
        inside[t] = 16 * tA < g.ldv && 16 * tB < g.ldv && tA <= tB;
        live[t] = inside[t] && 16 * tA < g.nv && 16 * tB < g.nv;
    }
    v4d acc1[4], acc2[4];
    mp2_sweep<4>(s_p, src, sld, scol, g, wave, l15, q, live, acc1, acc2);
    // epilogue: lane (l15, q), register r holds a = 16 tA + q + 4 r, b = 16 tB + l15 (acc1: V_ab, acc2: V_ba)
    const size_t ld = (size_t)g.ldv;
    double *ot = g.t + (size_t)pair * ld * ld, *ott = g.tt + (size_t)pair * ld * ld;
    const double eij = g.eo[i] + g.eo[j];
    double ea[4];
    bool oka[4];
    mp2_rows(g.ev, g.nv, tA, q, ea, oka);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (!inside[t]) continue;  // (wave-uniform)
        const int tB = 4 * pb + t, b = 16 * tB + l15;
        const bool okb = b < g.nv;
        const double eb = okb ? g.ev[b] : 0.0;
        double xt[4], yt[4];  // the transposed position's T and Tt
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool ok = oka[r] && okb;
            const double d = ok ? eij - (ea[r] + eb) : 1.0;
            const double x = ok ? acc1[t][r] / d : 0.0, y = ok ? acc2[t][r] / d : 0.0;
            const size_t o = (size_t)(16 * tA + q + 4 * r) * ld + b;
            ot[o] = x;
            ott[o] = ok ? g.c1 * x - g.c2 * y : 0.0;
            xt[r] = y;
            yt[r] = ok ? g.c1 * y - g.c2 * x : 0.0;
        }
        if (tA == tB) continue;
        // (b, a): through the scratch, then rows b = 16 tB + q + 4 r, 16 consecutive a per 16 lanes
        double m[4];
        tile_transpose(s_tr[wave], xt, m);
#pragma unroll
        for (int r = 0; r < 4; r++) ot[(size_t)(16 * tB + q + 4 * r) * ld + 16 * tA + l15] = m[r];
        tile_transpose(s_tr[wave], yt, m);
#pragma unroll
        for (int r = 0; r < 4; r++) ott[(size_t)(16 * tB + q + 4 * r) * ld + 16 * tA + l15] = m[r];
    }
}

// (occupied pairs, panel pairs per occupied pair); false: an argument is out of range
static bool mp2_counts(int noi, int noj, int nva, int nvb, int same, long long &npair, long long &ntp, int &npa, int &npb) {
    if (noi < 0 || noj < 0 || nva < 0 || nvb < 0) return false;
    if (same && (noi != noj || nva != nvb)) return false;
    npa = (nva + MP2_PW - 1) / MP2_PW;
    npb = (nvb + MP2_PW - 1) / MP2_PW;
    npair = same ? (long long)noi * (noi + 1) / 2 : (long long)noi * noj;
    ntp = same ? (long long)npa * (npa + 1) / 2 : (long long)npa * npb;
    return true;
}

}  // namespace dqc

extern "C" {

size_t dqc_mp2_work_doubles(int noi, int noj, int nva, int nvb, int same) {
    long long npair, ntp;
    int npa, npb;
    if (!dqc::mp2_counts(noi, noj, nva, nvb, same, npair, ntp, npa, npb)) return 0;
    return (size_t)(2 * npair * ntp);
}

int dqc_mp2_pair_energies(double *d_eos, double *d_ess, const double *d_bi, const double *d_bj, const double *d_eoi,
                          const double *d_eoj, const double *d_eva, const double *d_evb, int noi, int noj, int nva, int nvb,
                          int ldva, int ldvb, int naux, int same, double *d_work, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    if (noi < 0 || noj < 0 || nva < 0 || nvb < 0 || naux < 0) { set_error("dqc_mp2_pair_energies: negative count"); return DQC_EINVAL; }
    if (ldva % 16 || ldvb % 16 || ldva < nva || ldvb < nvb) {
        set_error("dqc_mp2_pair_energies: ldv must be a multiple of 16 and at least nv");
        return DQC_EINVAL;
    }
    if (same && (noi != noj || nva != nvb || ldva != ldvb)) {
        set_error("dqc_mp2_pair_energies: same mode needs equal shapes on both sides");
        return DQC_EINVAL;
    }
    long long npair, ntp;
    int npa, npb;
    mp2_counts(noi, noj, nva, nvb, same, npair, ntp, npa, npb);
    if (noi == 0 || noj == 0) return DQC_OK;  // (empty outputs)
    if (!d_eos || (same && !d_ess)) { set_error("dqc_mp2_pair_energies: null output"); return DQC_EINVAL; }
    if (nva == 0 || nvb == 0 || naux == 0) {
        DQC_HIP(hipMemsetAsync(d_eos, 0, sizeof(double) * (size_t)noi * noj, st));
        if (same) DQC_HIP(hipMemsetAsync(d_ess, 0, sizeof(double) * (size_t)noi * noj, st));
        return DQC_OK;
    }
    if (!d_bi || !d_bj || !d_eoi || !d_eoj || !d_eva || !d_evb || !d_work) {
        set_error("dqc_mp2_pair_energies: null pointer argument");
        return DQC_EINVAL;
    }
    if (same && d_bi != d_bj) { set_error("dqc_mp2_pair_energies: same mode takes one tensor on both sides"); return DQC_EINVAL; }
    if (npair * ntp > 2147483647LL) { set_error("dqc_mp2_pair_energies: more blocks than one launch holds"); return DQC_EINVAL; }
    Mp2Args g{d_bi, d_bj, d_eoi, d_eoj, d_eva, d_evb, d_work, noi, noj, nva, nvb, ldva, ldvb, naux, npa, npb, ntp};
    if (same)
        hipLaunchKernelGGL(mp2_pair_kernel<true>, dim3((unsigned)(npair * ntp)), dim3(256), 0, st, g);
    else
        hipLaunchKernelGGL(mp2_pair_kernel<false>, dim3((unsigned)(npair * ntp)), dim3(256), 0, st, g);
    DQC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mp2_sum_kernel, dim3((unsigned)((npair + 63) / 64)), dim3(64), 0, st, d_eos, d_ess, (const double *)d_work, npair,
                       ntp, noj, same);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

int dqc_mp2_amplitudes(double *d_t, double *d_tt, size_t out_doubles, const double *d_bov, const double *d_eo, const double *d_ev,
                       int nocc, int nv, int ldv, int naux, int i0, int ni, double c_os, double c_ss, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    if (nocc < 0 || nv < 0 || ldv < 0 || naux < 0 || i0 < 0 || ni < 0) { set_error("dqc_mp2_amplitudes: negative count"); return DQC_EINVAL; }
    if (ldv % 16 || ldv < nv) { set_error("dqc_mp2_amplitudes: ldv must be a multiple of 16 and at least nv"); return DQC_EINVAL; }
    if ((long long)i0 + ni > nocc) { set_error("dqc_mp2_amplitudes: the occupied block [i0, i0 + ni) leaves the occupied space"); return DQC_EINVAL; }
    const size_t need = (size_t)ni * (size_t)nocc * (size_t)ldv * (size_t)ldv;
    if (need > out_doubles) { set_error("dqc_mp2_amplitudes: the output buffers are smaller than ni * nocc * ldv * ldv doubles"); return DQC_EINVAL; }
    if (need == 0) return DQC_OK;  // (empty outputs)
    if (!d_t || !d_tt) { set_error("dqc_mp2_amplitudes: null output"); return DQC_EINVAL; }
    if (nv == 0 || naux == 0) {
        DQC_HIP(hipMemsetAsync(d_t, 0, sizeof(double) * need, st));
        DQC_HIP(hipMemsetAsync(d_tt, 0, sizeof(double) * need, st));
        return DQC_OK;
    }
    if (!d_bov || !d_eo || !d_ev) { set_error("dqc_mp2_amplitudes: null pointer argument"); return DQC_EINVAL; }
    if ((size_t)d_bov % 16) { set_error("dqc_mp2_amplitudes: the tensor must be 16-byte aligned"); return DQC_EINVAL; }
    const long long np = (ldv + MP2_PW - 1) / MP2_PW, ntp = np * (np + 1) / 2, nblk = (long long)ni * nocc * ntp;
    if (nblk > 2147483647LL) { set_error("dqc_mp2_amplitudes: more blocks than one launch holds"); return DQC_EINVAL; }
    Mp2AmpArgs g{d_bov, d_eo, d_ev, d_t, d_tt, c_os + c_ss, c_ss, nocc, nv, ldv, naux, i0, ntp};
    hipLaunchKernelGGL(mp2_amp_kernel, dim3((unsigned)nblk), dim3(256), 0, st, g);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

}  // extern "C"
