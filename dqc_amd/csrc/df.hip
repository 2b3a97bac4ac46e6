// df.hip -- 2-centre and 3-centre 2-electron integrals for density fitting.
// Replaces  intor.coul2c(auxbw) = int2c2e_sph  and  intor.coul3c(basisw, basisw, auxbw) = int3c2e_sph
// (reference call sites dqc/df/dfmol.py:35-40, dqc/hamilton/intor/molintor.py:36-72, 121-130, 624-665).
//
// libcint evaluates (ij|k) and (k|l) as 4-centre integrals whose missing functions are the unit s-function.  The
// same construction is used here: one extra shell with exponent 0 and coefficient sqrt(4 pi) (cancelling the l = 0
// solid-harmonic factor) is appended to the shell table, the ket "pair" list is (auxiliary shell, unit), and the
// Rys shell-quartet kernel of eri_core.hpp runs unchanged in its 3C / 2C output modes: <LA,LB,LC,0> and <LA,0,LC,0>.
#include "eri_generic.hpp"
#include "grid_common.hpp"

namespace dqc {

struct DfSetup {
    Basis b;
    HostPairs orb, aux;
    DevPool pool;
    DevShells ds;
    DevPairs dorb{nullptr, nullptr, nullptr}, daux{nullptr, nullptr, nullptr};
    EriOut og{0, 0, 0, 0};
};

static int df_setup(DfSetup &s, const int *atm, int natm, const int *bas, int nbas, const double *env, int nenv, int sh0,
                    int sh1, int k0, int k1, bool need_orb, hipStream_t st, const char *who) {
    int rc = parse_basis(s.b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    if ((rc = boys_table_ensure())) return rc;
    if (sh0 < 0 || sh1 > nbas || sh0 > sh1 || k0 < 0 || k1 > nbas || k0 > k1) {
        set_error(std::string(who) + ": shell ranges outside the table");
        return DQC_EINVAL;
    }
    auto ao_of = [&](int sh) { return sh < nbas ? s.b.shells[sh].ao_off : s.b.nao; };
    s.og.ao0 = ao_of(sh0);
    s.og.nao = ao_of(sh1) - ao_of(sh0);
    s.og.aux0 = ao_of(k0);
    s.og.naux = ao_of(k1) - ao_of(k0);
    const int unit = append_unit_shell(s.b, 3.5449077018110320546);  // sqrt(4 pi)
    if (need_orb) build_pairs(s.b, s.orb, sh0, sh1);
    build_pairs(s.b, s.aux, k0, k1, unit);
    if ((rc = upload_shells(s.ds, s.b, s.pool, st))) { set_error(std::string(who) + ": device upload failed"); return rc; }
    if (need_orb && (rc = upload_pairs(s.pool, s.orb, s.dorb, st))) { set_error(std::string(who) + ": device upload failed"); return rc; }
    if ((rc = upload_pairs(s.pool, s.aux, s.daux, st))) { set_error(std::string(who) + ": device upload failed"); return rc; }
    return 0;
}

template <int LA, int LB, int LC, int MODE>
static int launch_df_class(double *out, const DfSetup &s, hipStream_t st) {
    using Cfg = EriCfg<LA, LB, LC, 0>;
    const HostPairs &hb = MODE == ERI_OUT_3C ? s.orb : s.aux;
    const DevPairs &db = MODE == ERI_OUT_3C ? s.dorb : s.daux;
    const int cb = LA * (LA + 1) / 2 + LB, ck = LC * (LC + 1) / 2;
    const int nb = hb.cls_count[cb], nk = s.aux.cls_count[ck];
    if (nb == 0 || nk == 0 || hl_forced()) return 0;
    const long long ntask = (long long)nb * nk;
    const long long nblk = eri_num_blocks<Cfg>(nb, nk, ntask);
    auto kern = eri_kernel<LA, LB, LC, 0, MODE>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS_BYTES);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), Cfg::LDS_BYTES, st, out, s.ds, db, s.daux, hb.cls_start[cb],
                       nb, s.aux.cls_start[ck], nk, 0, ntask, s.og);
    DQC_CHECK_LAUNCH();
    return 0;
}

template <int LC>
static int launch_3c_ket(double *out, const DfSetup &s, hipStream_t st) {
    int rc;
#define DQC_3C(LA, LB) \
    if ((rc = launch_df_class<LA, LB, LC, ERI_OUT_3C>(out, s, st))) return rc;
    DQC_3C(0, 0) DQC_3C(1, 0) DQC_3C(1, 1) DQC_3C(2, 0) DQC_3C(2, 1) DQC_3C(2, 2) DQC_3C(3, 0) DQC_3C(3, 1) DQC_3C(3, 2)
    DQC_3C(3, 3)
#undef DQC_3C
    return 0;
}

template <int LC>
static int launch_2c_ket(double *out, const DfSetup &s, hipStream_t st) {
    int rc;
#define DQC_2C(LA) \
    if ((rc = launch_df_class<LA, 0, LC, ERI_OUT_2C>(out, s, st))) return rc;
    DQC_2C(0) DQC_2C(1) DQC_2C(2) DQC_2C(3)
#undef DQC_2C
    return 0;
}

// classes with a g shell (orbital or auxiliary) through the runtime kernel (eri_generic.hpp); DQC_ERI_GENERIC=1: all classes
template <int MODE>
static int launch_df_generic(double *out, const DfSetup &s, hipStream_t st) {
    const HostPairs &hb = MODE == ERI_OUT_3C ? s.orb : s.aux;
    const DevPairs &db = MODE == ERI_OUT_3C ? s.dorb : s.daux;
    for (int la = 0; la <= DQC_LMAX; la++)
        for (int lb = 0; lb <= (MODE == ERI_OUT_3C ? la : 0); lb++)
            for (int lc = 0; lc <= DQC_LMAX; lc++) {
                if (!hl_forced() && la <= ERI_LMAX && lc <= ERI_LMAX) continue;
                const int cb = la * (la + 1) / 2 + lb, ck = lc * (lc + 1) / 2;
                int rc = launch_hl<MODE>(out, s.ds, db, s.daux, hb.cls_start[cb], hb.cls_count[cb], s.aux.cls_start[ck],
                                         s.aux.cls_count[ck], 0, s.og, la, lb, lc, 0, st);
                if (rc) return rc;
            }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// density-fitted Coulomb matrix from the stored integrals (DFMol.get_elrep, dfmol.py:60-79):
//     t_k = sum_ij D_ij (ij|k),   c = (k|l)^-1 t,   J_ij = sum_k (ij|k) c_k
// Both passes stream j3c once; (ij|k) = (ji|k), so only the rows i >= j of the (nao, nao, naux) array are read
// (half the bytes) and D enters as (D_ij + D_ji)(1 - delta_ij / 2).  HBM-bound: 2 x 4 nao (nao+1) naux bytes.
// ---------------------------------------------------------------------------------------------
DQC_DEV void tri_decode(long long q, int &i, int &j) {
    long long r = (long long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > q) r--;
    while ((r + 1) * (r + 2) / 2 <= q) r++;
    i = (int)r;
    j = (int)(q - r * (r + 1) / 2);
}

constexpr int DF_ROWS = 64;  // triangular rows per block in the first pass (32: twice the atomics on the naux sums, 0.113 ms; 64: 0.087; 96: 0.089 -- C5 molecule)

__global__ __launch_bounds__(256) void df_rhs_kernel(double *__restrict__ t, const double *__restrict__ j3c,
                                                     const double *__restrict__ dm, int nao, int naux, long long npair) {
    __shared__ double sw[DF_ROWS];
    __shared__ long long soff[DF_ROWS];
    const long long q0 = (long long)blockIdx.x * DF_ROWS;
    if (threadIdx.x < DF_ROWS) {
        const long long q = q0 + threadIdx.x;
        double wgt = 0.0;
        long long off = 0;
        if (q < npair) {
            int i, j;
            tri_decode(q, i, j);
            wgt = (dm[(size_t)i * nao + j] + dm[(size_t)j * nao + i]) * (i == j ? 0.5 : 1.0);
            off = ((long long)i * nao + j) * naux;
        }
        sw[threadIdx.x] = wgt;
        soff[threadIdx.x] = off;
    }
    __syncthreads();
    if ((naux & 1) == 0) {  // rows are 16-byte aligned: two auxiliary functions per lane and load
        for (int k = 2 * threadIdx.x; k < naux; k += 512) {
            double a0 = 0.0, a1 = 0.0;
#pragma unroll 8
            for (int r = 0; r < DF_ROWS; r++) {
                const double2 v = *reinterpret_cast<const double2 *>(j3c + soff[r] + k);
                a0 += sw[r] * v.x;
                a1 += sw[r] * v.y;
            }
            atomicAdd(&t[k], a0);
            atomicAdd(&t[k + 1], a1);
        }
        return;
    }
    for (int k = threadIdx.x; k < naux; k += 256) {
        double acc = 0.0;
#pragma unroll 8
        for (int r = 0; r < DF_ROWS; r++) acc += sw[r] * j3c[soff[r] + k];
        atomicAdd(&t[k], acc);
    }
}

// y = A x for a small dense (n, n) matrix: one wave per row
__global__ __launch_bounds__(256) void df_matvec_kernel(double *__restrict__ y, const double *__restrict__ a,
                                                        const double *__restrict__ x, int n) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) acc += a[(size_t)row * n + k] * x[k];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) y[row] = acc;
}

__global__ __launch_bounds__(256) void df_j_kernel(double *__restrict__ jmat, const double *__restrict__ j3c,
                                                   const double *__restrict__ c, int nao, int naux, long long npair) {
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= npair) return;
    int i, j;
    tri_decode(q, i, j);
    const double *row = j3c + ((size_t)i * nao + j) * naux;
    double acc = 0.0;
    if ((naux & 1) == 0) {
        // four loads of the row in flight per lane (the plain loop waited for every 16 bytes before asking for the next: a 9 KB row
        // was nine dependent round trips)
        int k = 2 * lane;
        double a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (; k + 384 < naux; k += 512) {
            const double2 v0 = *reinterpret_cast<const double2 *>(row + k), v1 = *reinterpret_cast<const double2 *>(row + k + 128);
            const double2 v2 = *reinterpret_cast<const double2 *>(row + k + 256), v3 = *reinterpret_cast<const double2 *>(row + k + 384);
            const double2 c0 = *reinterpret_cast<const double2 *>(c + k), c1 = *reinterpret_cast<const double2 *>(c + k + 128);
            const double2 c2 = *reinterpret_cast<const double2 *>(c + k + 256), c3 = *reinterpret_cast<const double2 *>(c + k + 384);
            acc += v0.x * c0.x + v0.y * c0.y;
            a1 += v1.x * c1.x + v1.y * c1.y;
            a2 += v2.x * c2.x + v2.y * c2.y;
            a3 += v3.x * c3.x + v3.y * c3.y;
        }
        for (; k < naux; k += 128) {
            const double2 v = *reinterpret_cast<const double2 *>(row + k), cc = *reinterpret_cast<const double2 *>(c + k);
            acc += v.x * cc.x + v.y * cc.y;
        }
        acc += a1 + a2 + a3;
    } else
        for (int k = lane; k < naux; k += 64) acc += row[k] * c[k];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) {
        jmat[(size_t)i * nao + j] = acc;
        jmat[(size_t)j * nao + i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// density-fitted exchange (RI-K) from the Cholesky-whitened three-index tensor B[P, mu, nu] = sum_Q (L^-1)[P, Q] (mu nu|Q):
//     Y[P, mu, i] = sum_lam B[P, mu, lam] Lf[lam, i],     K[mu, nu] = sum_P sum_i Y[P, mu, i] Y[P, nu, i],     D = Lf Lf^T
//
// Stage 1, df_k_half_kernel: the tall-skinny GEMM (naux nao) x nao x rp on the fp64 matrix cores.  One wave owns two 16-row
// tiles of one or two slabs B_P and all rp / 16 column tiles; B streams from HBM straight into the MFMA operand registers -- lane
// (j, q) loads the four consecutive doubles B[P, mu0 + j, k0 + 4 q .. + 3] (32 contiguous bytes per lane, 128 per row) and feeds
// them to four MFMAs whose k index it defines as k0 + 4 q + s; the factor operand is read from LDS under the same map, so the
// permutation of k inside a 16-block cancels and B is never staged or read twice.  Lf is staged in LDS in chunks of DFK_LDS_DOUBLES
// (row stride rp + 4 == 4 (mod 8): the two k rows a 32-lane half reads sit 32 banks apart, ds_read_b64 conflict-free), each element
// once per block.  The product is formed TRANSPOSED -- Lf^T as the A operand, B_P^T as the B operand -- so that the accumulator has
// mu on the lane (C[row = i][col = mu]) and Y is written as the matrix stage 2 wants:  Yt[(P, i), mu], row stride lda =
// dqc_ao_stride(nao), 128 contiguous bytes per 16 lanes.  No cross-block sums: bit-reproducible as it stands.
//
// Stage 2, K = Yt^T Yt, is the split-K symmetric rank update of the Vxc pass with (P, i) in the role of the grid points and unit
// weights -- dqc_grid_vxc's one-operand form as it is (grid_vxc.hip: producer / consumer waves, upper-triangular tiles for nao <= 240,
// fp64 atomics or, in deterministic mode, fixed point on 2^47, the closing symmetrisation that also zeroes the padding).
// ---------------------------------------------------------------------------------------------
constexpr int DFK_LDS_DOUBLES = 8192;  // 64 KB of factor rows per chunk: two blocks per CU, i.e. two MFMA-issuing waves per SIMD

DQC_DEV void dfk_load4(double (&a)[4], const double *row, int k, int nao, bool ok, bool even) {
    // row[k .. k + 3], zero past the end of the row (and for a row that does not exist)
    if (ok && even && k + 3 < nao) {  // (even nao: every row starts on 16 bytes)
        const double2 v0 = *reinterpret_cast<const double2 *>(row + k), v1 = *reinterpret_cast<const double2 *>(row + k + 2);
        a[0] = v0.x; a[1] = v0.y; a[2] = v1.x; a[3] = v1.y;
    } else {
#pragma unroll
        for (int s = 0; s < 4; s++) a[s] = ok && k + s < nao ? row[k + s] : 0.0;
    }
}

template <int NT>  // NT = rp / 16 column tiles of the factor
__global__ __launch_bounds__(256, 2) void df_k_half_kernel(double *__restrict__ yt, const double *__restrict__ b,
                                                           const double *__restrict__ orb, int nao, int naux, int ld, int lda, int kc) {
    extern __shared__ __align__(16) double s_lf[];  // [kc][rp + 4]
    constexpr int RP = 16 * NT, LS = RP + 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int T = ld >> 4;
    const long long ntile = (long long)naux * T;
    const bool even = (nao & 1) == 0;
    const double *row[2];
    bool ok[2];
    long long tile[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        tile[u] = ((long long)blockIdx.x * 4 + wave) * 2 + u;
        const long long tt = tile[u] < ntile ? tile[u] : 0;
        const int p = (int)(tt / T), mu = (int)(tt - (long long)p * T) * 16 + j;
        ok[u] = tile[u] < ntile && mu < nao;
        row[u] = b + ((size_t)p * nao + (ok[u] ? mu : 0)) * nao;
    }
    v4d acc[2][NT];
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[u][t] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < ld; c0 += kc) {
        const int cn = min(kc, ld - c0);  // (multiples of 16; rows nao .. ld - 1 of the padded factor are zero)
        __syncthreads();
        for (int e = threadIdx.x * 2; e < cn * RP; e += 512) {
            const int k = e / RP, i = e - k * RP;
            const double2 v = *reinterpret_cast<const double2 *>(orb + (size_t)(c0 + k) * RP + i);
            *reinterpret_cast<double2 *>(&s_lf[k * LS + i]) = v;
        }
        __syncthreads();
        double a[2][4];
        dfk_load4(a[0], row[0], c0 + 4 * q, nao, ok[0], even);
        dfk_load4(a[1], row[1], c0 + 4 * q, nao, ok[1], even);
        for (int k0 = 0; k0 < cn; k0 += 16) {
            double an[2][4];  // the next k-block's rows are asked for before this block's MFMAs
            const int kn = c0 + k0 + 16 + 4 * q;
            const bool more = k0 + 16 < cn;
            dfk_load4(an[0], row[0], kn, nao, ok[0] && more, even);
            dfk_load4(an[1], row[1], kn, nao, ok[1] && more, even);
            const double *lf = s_lf + (k0 + 4 * q) * LS + j;
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const double f = lf[s * LS + 16 * t];
                    acc[0][t] = mfma_f64(f, a[0][s], acc[0][t]);
                    acc[1][t] = mfma_f64(f, a[1][s], acc[1][t]);
                }
#pragma unroll
            for (int s = 0; s < 4; s++) { a[0][s] = an[0][s]; a[1][s] = an[1][s]; }
        }
    }
    // C[row = q + 4 reg][col = j]: factor column i = 16 t + q + 4 reg, AO mu = 16 tmu + j
#pragma unroll
    for (int u = 0; u < 2; u++) {
        if (tile[u] >= ntile) continue;
        const int p = (int)(tile[u] / T), mu = (int)(tile[u] - (long long)p * T) * 16 + j;
        if (mu >= lda) continue;  // (columns nao .. lda - 1 receive the zeros of the rows that do not exist)
        double *out = yt + (size_t)p * RP * lda + mu;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) out[(size_t)(16 * t + q + 4 * r) * lda] = acc[u][t][r];
    }
}

// the unit weights of stage 2 and the slack behind Yt that the Vxc kernels' 16-column tile reads reach
__global__ void df_k_fill_kernel(double *__restrict__ slack, int nslack, double *__restrict__ ones, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ones[i] = 1.0;
    if (i < nslack) slack[i] = 0.0;
}

template <int NT>
static void launch_df_k_half(double *yt, const double *b, const double *orb, int nao, int naux, int ld, int lda, hipStream_t st) {
    const int rp = 16 * NT;
    const int kc = std::min(ld, DFK_LDS_DOUBLES / (rp + 4) / 16 * 16);
    const size_t shmem = sizeof(double) * (size_t)kc * (rp + 4);
    const long long ntile = (long long)naux * (ld / 16);
    auto kern = df_k_half_kernel<NT>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL(kern, dim3((unsigned)((ntile + 7) / 8)), dim3(256), shmem, st, yt, b, orb, nao, naux, ld, lda, kc);
}

}  // namespace dqc

extern "C" {

int dqc_int3c2e(double *d_out, const int *atm, int natm, const int *bas, int nbas, const double *env, int nenv, int sh0,
                int sh1, int k0, int k1, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    DfSetup s;
    int rc = df_setup(s, atm, natm, bas, nbas, env, nenv, sh0, sh1, k0, k1, true, st, "dqc_int3c2e");
    if (rc) return rc;
    if (s.og.nao == 0 || s.og.naux == 0) return DQC_OK;
    if ((rc = launch_3c_ket<0>(d_out, s, st)) || (rc = launch_3c_ket<1>(d_out, s, st)) ||
        (rc = launch_3c_ket<2>(d_out, s, st)) || (rc = launch_3c_ket<3>(d_out, s, st)) ||
        (rc = launch_df_generic<ERI_OUT_3C>(d_out, s, st)))
        return rc;
    DQC_HIP(hipStreamSynchronize(st));
    return DQC_OK;
}

int dqc_int2c2e(double *d_out, const int *atm, int natm, const int *bas, int nbas, const double *env, int nenv, int k0,
                int k1, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    DfSetup s;
    int rc = df_setup(s, atm, natm, bas, nbas, env, nenv, 0, 0, k0, k1, false, st, "dqc_int2c2e");
    if (rc) return rc;
    if (s.og.naux == 0) return DQC_OK;
    if ((rc = launch_2c_ket<0>(d_out, s, st)) || (rc = launch_2c_ket<1>(d_out, s, st)) ||
        (rc = launch_2c_ket<2>(d_out, s, st)) || (rc = launch_2c_ket<3>(d_out, s, st)) ||
        (rc = launch_df_generic<ERI_OUT_2C>(d_out, s, st)))
        return rc;
    DQC_HIP(hipStreamSynchronize(st));
    return DQC_OK;
}

int dqc_df_coulomb(double *d_j, const double *d_j3c, const double *d_inv_j2c, const double *d_dm_ao, int nao, int naux,
                   double *d_work, void *stream) {
    // d_work: 2 * naux doubles (t, c); d_j (nao, nao) is overwritten.  Enqueues only.
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    if (nao <= 0) return DQC_OK;
    if (naux <= 0) { DQC_HIP(hipMemsetAsync(d_j, 0, sizeof(double) * (size_t)nao * nao, st)); return DQC_OK; }
    const long long npair = (long long)nao * (nao + 1) / 2;
    double *t = d_work, *c = d_work + naux;
    DQC_HIP(hipMemsetAsync(t, 0, sizeof(double) * naux, st));
    hipLaunchKernelGGL(df_rhs_kernel, dim3((unsigned)((npair + DF_ROWS - 1) / DF_ROWS)), dim3(256), 0, st, t, d_j3c, d_dm_ao,
                       nao, naux, npair);
    DQC_CHECK_LAUNCH();
    hipLaunchKernelGGL(df_matvec_kernel, dim3((unsigned)((naux + 3) / 4)), dim3(256), 0, st, c, d_inv_j2c, t, naux);
    DQC_CHECK_LAUNCH();
    hipLaunchKernelGGL(df_j_kernel, dim3((unsigned)((npair + 3) / 4)), dim3(256), 0, st, d_j, d_j3c, c, nao, naux, npair);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

size_t dqc_df_exchange_work_doubles(int nao, int naux, int rp) {
    // Yt (naux rp rows of dqc_ao_stride(nao) doubles) | 16 doubles of slack | naux rp unit weights
    if (nao <= 0 || naux <= 0 || rp <= 0) return 0;
    return (size_t)naux * rp * dqc_ao_stride(nao) + 16 + (size_t)naux * rp;
}

int dqc_df_exchange(double *d_k, const double *d_b, const double *d_orb, const double *d_orbt, int nao, int naux, int rp,
                    double *d_work, void *stream) {
    // d_k (ld, ld), ld = dqc_padded_nao(nao), is overwritten (symmetric, zero padding).  Enqueues only.
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    (void)d_orbt;  // (the transposed half of the factor pair: this kernel stages the factor from d_orb alone)
    if (nao < 0 || naux < 0) { set_error("dqc_df_exchange: negative nao or naux"); return DQC_EINVAL; }
    if (rp <= 0 || dqc_padded_norb(rp) != rp) { set_error("dqc_df_exchange: rp is not a padded factor width (dqc_padded_norb)"); return DQC_EINVAL; }
    if (nao == 0) return DQC_OK;
    if (!d_k) { set_error("dqc_df_exchange: null output"); return DQC_EINVAL; }
    const int ld = dqc_padded_nao(nao), lda = dqc_ao_stride(nao);
    if (naux == 0) { DQC_HIP(hipMemsetAsync(d_k, 0, sizeof(double) * (size_t)ld * ld, st)); return DQC_OK; }
    if (!d_b || !d_orb || !d_work) { set_error("dqc_df_exchange: null pointer argument"); return DQC_EINVAL; }
    if ((long long)naux * rp > 2147483647LL / 2) { set_error("dqc_df_exchange: naux * rp beyond the row count of the rank update"); return DQC_EINVAL; }
    const int nrow = naux * rp;
    double *yt = d_work, *slack = yt + (size_t)nrow * lda, *ones = slack + 16;
    hipLaunchKernelGGL(df_k_fill_kernel, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, st, slack, 16, ones, nrow);
    DQC_CHECK_LAUNCH();
    switch (rp / 16) {
        case 1: launch_df_k_half<1>(yt, d_b, d_orb, nao, naux, ld, lda, st); break;
        case 2: launch_df_k_half<2>(yt, d_b, d_orb, nao, naux, ld, lda, st); break;
        case 3: launch_df_k_half<3>(yt, d_b, d_orb, nao, naux, ld, lda, st); break;
        case 4: launch_df_k_half<4>(yt, d_b, d_orb, nao, naux, ld, lda, st); break;
        case 6: launch_df_k_half<6>(yt, d_b, d_orb, nao, naux, ld, lda, st); break;
        case 8: launch_df_k_half<8>(yt, d_b, d_orb, nao, naux, ld, lda, st); break;
        default: set_error("dqc_df_exchange: no kernel for this factor width"); return DQC_EINVAL;
    }
    DQC_CHECK_LAUNCH();
    return dqc_grid_vxc(d_k, yt, 1, nrow, nao, ones, ones, nullptr, stream);
}

}  // extern "C"
