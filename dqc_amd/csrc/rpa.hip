// rpa.hip -- the RI-dRPA response matrix on a grid of imaginary frequencies, fused: no frequency-scaled copy of the tensor is ever stored.
//
//     Q[k, P, R] (+)= scale * sum_i sum_{a < nv} Bov[i, P, a] g_ia(w_k) Bov[i, R, a],     g_ia(w) = D_ia / (D_ia^2 + w^2),  D_ia = ev[a] - eo[i]
//
// Bov[i, P, a]: one (naux, ldv) slab per occupied orbital, ldv the virtual count padded to a multiple of 16 (what mp2.transform_ov makes).
// A weighted symmetric rank-k update per frequency: the contraction index is the pair (i, a), a the CONTIGUOUS index of the tensor (in
// mp2.hip it is the row index P), and the weight depends on the frequency, so one staged operand serves every frequency of a group.
//
// One block (four waves) owns one 64 x 64 panel pair (Pp >= Rp) of Q, one group of RPA_NF frequencies and one slot of the (i, a) sum;
// wave w owns tile row P = 4 Pp + w and the four tiles R = 4 Rp + t of it, for all RPA_NF frequencies: RPA_NF x 4 accumulators of
// v_mfma_f64_16x16x4_f64.  The (i, a) sum runs in chunks of one occupied orbital and RPA_KC = 16 virtuals: the block stages the rows of
// the two panels [row][a] in LDS (each element read from memory once per block; the next chunk is asked for before the MFMAs of this one
// and stored after them) and the RPA_NF x 16 weights g of the chunk once (64 divisions per chunk and block).  Per k-step of four virtuals
// a lane reads its A value, its four B values and its RPA_NF weights, forms A g_f per frequency and issues RPA_NF x 4 MFMAs: 5 operand
// reads (and one read of the weights) feed 16 MFMAs.
// LDS row stride 18 doubles (== 2 mod 32): the fragment read [row = lane & 15][k = lane >> 4] of a 32-lane half touches the doubles
// 18 (lane & 15) + {0, 1}: the multiples of 18 are the 16 even residues mod 32, so the 32 addresses sit on 32 different 8-byte banks --
// conflict-free with ds_read_b64.  (The other route, one library transpose of Bov and the staging of mp2_pair_kernel, costs a second
// copy of the largest tensor of the calculation; this one costs nothing.)
//
// Lower triangle only: panel pairs Pp >= Rp, in a diagonal pair tiles P >= R, in a diagonal tile elements p >= r; the mirror element is
// written from the same register (off-diagonal tiles through a 16 x 17 LDS scratch per wave, so that every store instruction of a wave is
// four full 128-byte rows): Q[k] is bit-symmetric.
// Padding: columns a >= nv are staged as 0.0 (selected, not multiplied) and chunks that hold no real virtual are not visited; rows past
// naux are staged as 0.0 and never stored; the weights of the frequencies past nfreq in the last group are 0.0 and their tiles are not
// stored.  Whatever the padding holds, it contributes exactly zero.
// No atomics.  slots == 1: every element of Q is written (accumulate: read, added to, written) by one lane.  slots > 1 (few panel pairs:
// the (i, a) chunks are split over blocks for occupancy): every block writes its raw partial sums to its slot of the work buffer and
// rpa_sum_kernel adds the slots of an element in slot order, scales, mirrors.  Bit-reproducible as it stands.
#include <algorithm>

#include "common.hpp"
#include "mfma_tile.hpp"

namespace dqc {

constexpr int RPA_NF = 4;    // frequencies in flight per block (4 x 4 tiles x 8 = 128 accumulator VGPRs per lane)
constexpr int RPA_KC = 16;   // virtuals per LDS chunk
constexpr int RPA_PW = 64;   // panel width (four tiles)
constexpr int RPA_LS = 18;   // LDS row stride in doubles
constexpr long long RPA_TARGET_BLOCKS = 1024;       // the (i, a) sum is split while the launch has fewer blocks than this
constexpr long long RPA_WORK_CAP = 1LL << 24;       // doubles: the work buffer never exceeds this (the host splits less)

struct RpaArgs {
    const double *bov, *eo, *ev, *freq;
    double *q, *part;    // part: [slot][k][P][R], raw sums of the lower triangle (slots > 1)
    double scale;
    int nocc, nv, ldv, naux, nfreq, accumulate;
    int nca;             // chunks per occupied orbital: ceil(nv / 16)
    int nfg;             // frequency groups
    int slots, cps;      // slots of the (i, a) sum, chunks per slot
    long long ntp;       // panel pairs
};

__global__ __launch_bounds__(256, 2) void rpa_response_kernel(RpaArgs g) {
    __shared__ __align__(16) double s_p[2][RPA_PW][RPA_LS];     // [P panel, R panel][row][a]
    __shared__ __align__(16) double s_g[RPA_KC][RPA_NF];        // the weights of the chunk
    __shared__ double s_tr[4][16][17];                          // per wave: one tile on its way to the mirrored position
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    long long b = blockIdx.x;
    const int kg = (int)(b % g.nfg);
    b /= g.nfg;
    const long long tp = b % g.ntp;
    const int slot = (int)(b / g.ntp);
    int pr, pp;
    tri_index(tp, pr, pp);   // pr <= pp
    const int tP = 4 * pp + wave;
    bool live[4];          // tiles this wave forms: inside the matrix, on or below the diagonal
#pragma unroll
    for (int t = 0; t < 4; t++) live[t] = 16 * tP < g.naux && 4 * pr + t <= tP;   // (tR <= tP: 16 tR < naux follows)
    const bool any = live[0] || live[1] || live[2] || live[3];
    v4d acc[RPA_NF][4];
#pragma unroll
    for (int f = 0; f < RPA_NF; f++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[f][t] = v4d{0.0, 0.0, 0.0, 0.0};

    // the staging map: 64 rows x 8 double2 per panel = 512 double2, two per thread and panel; threads 0 ... 63 one weight each
    const int grow[2] = {pp * RPA_PW, pr * RPA_PW};
    const int ga = threadIdx.x / RPA_NF, gf = threadIdx.x % RPA_NF, gk = RPA_NF * kg + gf;   // (ga < 16 for the first 64 threads)
    const double w2 = (threadIdx.x < RPA_KC * RPA_NF && gk < g.nfreq) ? g.freq[gk] * g.freq[gk] : 0.0;
    double2 nx[2][2];
    double ng = 0.0;
    auto fetch = [&](int c) {
        const int i = c / g.nca, a0 = RPA_KC * (c - i * g.nca);
        const double *slab = g.bov + (size_t)i * g.naux * g.ldv;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = threadIdx.x + 256 * u, row = grow[p] + (e >> 3), a = a0 + (e & 7) * 2;
                double2 v{0.0, 0.0};
                if (row < g.naux) v = *reinterpret_cast<const double2 *>(slab + (size_t)row * g.ldv + a);   // (a + 1 < ldv: whole 16s)
                nx[p][u] = double2{a < g.nv ? v.x : 0.0, a + 1 < g.nv ? v.y : 0.0};
            }
        if (threadIdx.x < RPA_KC * RPA_NF) {
            const int a = a0 + ga;
            const bool ok = a < g.nv && gk < g.nfreq;
            const double d = ok ? g.ev[a] - g.eo[i] : 1.0;
            ng = ok ? d / (d * d + w2) : 0.0;
        }
    };
    const int c_lo = slot * g.cps, c_hi = min(c_lo + g.cps, g.nocc * g.nca);
    if (c_lo < c_hi) fetch(c_lo);
    for (int c = c_lo; c < c_hi; c++) {
        __syncthreads();  // (the previous chunk has been read by every wave)
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = threadIdx.x + 256 * u;
                *reinterpret_cast<double2 *>(&s_p[p][e >> 3][(e & 7) * 2]) = nx[p][u];
            }
        if (threadIdx.x < RPA_KC * RPA_NF) s_g[ga][gf] = ng;
        __syncthreads();
        if (c + 1 < c_hi) fetch(c + 1);
        if (!any) continue;
#pragma unroll
        for (int k0 = 0; k0 < RPA_KC; k0 += 4) {
            const double a = s_p[0][16 * wave + l15][k0 + q];
            double bt[4], af[RPA_NF];
#pragma unroll
            for (int t = 0; t < 4; t++) bt[t] = s_p[1][16 * t + l15][k0 + q];
#pragma unroll
            for (int f = 0; f < RPA_NF; f++) af[f] = a * s_g[k0 + q][f];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (!live[t]) continue;  // (wave-uniform)
#pragma unroll
                for (int f = 0; f < RPA_NF; f++) acc[f][t] = mfma_f64(af[f], bt[t], acc[f][t]);
            }
        }
    }
    if (!any) return;   // (no block-wide barrier below)
    // epilogue: lane (l15, q), register r holds row p = 16 tP + q + 4 r, column rc = 16 tR + l15
    const size_t n = (size_t)g.naux, nn = n * n;
#pragma unroll
    for (int f = 0; f < RPA_NF; f++) {
        const int k = RPA_NF * kg + f;
        if (k >= g.nfreq) continue;  // (block-uniform)
        if (g.slots > 1) {           // raw partial sums of the lower triangle; rpa_sum_kernel scales and mirrors
            double *o = g.part + ((size_t)slot * g.nfreq + k) * nn;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (!live[t]) continue;
                const int rc = 16 * (4 * pr + t) + l15;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int p = 16 * tP + q + 4 * r;
                    if (p < g.naux && rc <= p) o[(size_t)p * n + rc] = acc[f][t][r];
                }
            }
            continue;
        }
        double *o = g.q + (size_t)k * nn;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (!live[t]) continue;  // (wave-uniform)
            const int tR = 4 * pr + t, rc = 16 * tR + l15;
            double v[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int p = 16 * tP + q + 4 * r;
                v[r] = g.scale * acc[f][t][r];
                if (p < g.naux && rc <= p) {   // (rc <= p < naux; off-diagonal tiles: always rc < p)
                    double *x = o + (size_t)p * n + rc;
                    *x = g.accumulate ? *x + v[r] : v[r];
                }
            }
            // (rc', p'): through the scratch, then rows rc' = 16 tR + q + 4 r of the mirror image, 16 consecutive p' = 16 tP + l15 per
            // 16 lanes; the diagonal itself was written above
            double m[4];
            tile_transpose(s_tr[wave], v, m);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int rc2 = 16 * tR + q + 4 * r, p2 = 16 * tP + l15;
                if (p2 < g.naux && rc2 < p2) {
                    double *x = o + (size_t)rc2 * n + p2;
                    *x = g.accumulate ? *x + m[r] : m[r];
                }
            }
        }
    }
}

// the slots of an element (p >= r) in slot order, scaled, written (or added) to both triangles
__global__ __launch_bounds__(256) void rpa_sum_kernel(double *__restrict__ q, const double *__restrict__ part, int naux, int nfreq, int slots,
                                                      double scale, int accumulate) {
    const size_t n = (size_t)naux, nn = n * n, tot = nn * (size_t)nfreq;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const size_t k = e / nn, pr = e - k * nn, p = pr / n, r = pr - p * n;
    if (r > p) return;
    double s = 0.0;
    for (int sl = 0; sl < slots; sl++) s += part[(size_t)sl * tot + e];
    s *= scale;
    double *x = q + e, *y = q + k * nn + r * n + p;
    if (accumulate) {
        const double vx = *x + s;
        if (r != p) *y = *y + s;
        *x = vx;
    } else {
        *x = s;
        if (r != p) *y = s;
    }
}

// (panel pairs, frequency groups, chunks per occupied orbital, slots, chunks per slot) of a launch; false: an argument is out of range
static bool rpa_counts(int nocc, int nv, int naux, int nfreq, long long &ntp, int &nfg, int &nca, int &slots, int &cps) {
    if (nocc < 0 || nv < 0 || naux < 0 || nfreq < 0) return false;
    const long long np = (naux + RPA_PW - 1) / RPA_PW;
    ntp = np * (np + 1) / 2;
    nfg = (nfreq + RPA_NF - 1) / RPA_NF;
    nca = (nv + RPA_KC - 1) / RPA_KC;
    slots = 1;
    cps = 0;
    const long long nchunk = (long long)nocc * nca, blocks = ntp * nfg;
    if (nchunk == 0 || blocks == 0) return true;
    long long s = blocks >= RPA_TARGET_BLOCKS ? 1 : (RPA_TARGET_BLOCKS + blocks - 1) / blocks;
    const long long per = (long long)nfreq * naux * naux;   // doubles per slot
    s = std::min(s, std::max(1LL, RPA_WORK_CAP / per));
    s = std::min(s, nchunk);
    const long long c = (nchunk + s - 1) / s;
    if (c > 2147483647LL) return false;
    cps = (int)c;
    slots = (int)((nchunk + c - 1) / c);   // (no empty slot)
    return true;
}

}  // namespace dqc

extern "C" {

size_t dqc_rpa_work_doubles(int nocc, int nv, int naux, int nfreq) {
    long long ntp;
    int nfg, nca, slots, cps;
    if (!dqc::rpa_counts(nocc, nv, naux, nfreq, ntp, nfg, nca, slots, cps)) return 0;
    return slots > 1 ? (size_t)slots * (size_t)nfreq * (size_t)naux * (size_t)naux : 0;
}

int dqc_rpa_response(double *d_q, const double *d_bov, const double *d_eo, const double *d_ev, const double *d_freq, int nocc, int nv,
                     int ldv, int naux, int nfreq, double scale, int accumulate, double *d_work, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    if (nocc < 0 || nv < 0 || ldv < 0 || naux < 0 || nfreq < 0) { set_error("dqc_rpa_response: negative count"); return DQC_EINVAL; }
    if (ldv % 16 || ldv < nv) { set_error("dqc_rpa_response: ldv must be a multiple of 16 and at least nv"); return DQC_EINVAL; }
    if (accumulate != 0 && accumulate != 1) { set_error("dqc_rpa_response: accumulate must be 0 or 1"); return DQC_EINVAL; }
    long long ntp;
    int nfg, nca, slots, cps;
    if (!rpa_counts(nocc, nv, naux, nfreq, ntp, nfg, nca, slots, cps)) { set_error("dqc_rpa_response: more chunks than one slot holds"); return DQC_EINVAL; }
    const size_t out = (size_t)nfreq * (size_t)naux * (size_t)naux;
    if (out == 0) return DQC_OK;  // (empty output)
    if (!d_q) { set_error("dqc_rpa_response: null output"); return DQC_EINVAL; }
    if (nocc == 0 || nv == 0) {   // an empty sum: zeros, or Q as it is
        if (!accumulate) DQC_HIP(hipMemsetAsync(d_q, 0, sizeof(double) * out, st));
        return DQC_OK;
    }
    if (!d_bov || !d_eo || !d_ev || !d_freq || (slots > 1 && !d_work)) { set_error("dqc_rpa_response: null pointer argument"); return DQC_EINVAL; }
    if ((size_t)d_bov % 16) { set_error("dqc_rpa_response: the tensor must be 16-byte aligned"); return DQC_EINVAL; }
    const long long nblk = ntp * nfg * slots;
    if (nblk > 2147483647LL) { set_error("dqc_rpa_response: more blocks than one launch holds"); return DQC_EINVAL; }
    const size_t nsum = (out + 255) / 256;   // (slots > 1: out <= RPA_WORK_CAP / 2)
    RpaArgs g{d_bov, d_eo, d_ev, d_freq, d_q, d_work, scale, nocc, nv, ldv, naux, nfreq, accumulate, nca, nfg, slots, cps, ntp};
    hipLaunchKernelGGL(rpa_response_kernel, dim3((unsigned)nblk), dim3(256), 0, st, g);
    DQC_CHECK_LAUNCH();
    if (slots > 1) {
        hipLaunchKernelGGL(rpa_sum_kernel, dim3((unsigned)nsum), dim3(256), 0, st, d_q, (const double *)d_work, naux, nfreq, slots, scale,
                           accumulate);
        DQC_CHECK_LAUNCH();
    }
    return DQC_OK;
}

}  // extern "C"
