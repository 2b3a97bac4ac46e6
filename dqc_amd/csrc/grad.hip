// grad.hip -- nuclear gradients of the SCF energy: the integral-derivative contractions.
//
// The reference obtains dE/dR by autograd through its integral wrappers (the "ip" derivative integrals,
// dqc/hamilton/intor/molintor.py:463-500) and the implicit-function backward of the SCF fixed point
// (dqc/qccalc/scf_qccalc.py:63-67, 109-113).  At a converged SCF point that derivative is the classic
// Hellmann-Feynman + Pulay expression, which needs no response equations:
//     dE/dR_A = sum D dh/dR_A - sum W dS/dR_A + 1/2 sum D D d(ab|cd)/dR_A [J - K/2 weights] + dE_xc/dR_A + dE_nn/dR_A
// This file provides the two integral-derivative terms, contracted on the fly (no derivative tensor is stored):
//   dqc_eri_grad   : g_A = sum_{a in A} sum_bcd (d_A a b|c d) [2 j D_ab D_cd - k D_ac D_bd]
//   dqc_int1e_grad : g_A = 2 sum_{a in A} sum_b [D_ab (d_A a|T + V|b) - W_ab (d_A a|b)],  g_C -= 2 sum_ab D_ab (d_A a|v_C|b)
// d/dA of a contracted Cartesian Gaussian of angular momentum l is an (l+1)-shell with coefficients 2 alpha c minus
// an (l-1)-shell; the 2e term therefore reuses the Rys shell-quartet kernel unchanged, with those companion shells
// first in the bra pair, in its GRAD output mode (eri_core.hpp).  Densities enter in the Cartesian AO basis
// (D_cart = T^T D T, T = dqc_cart2sph_matrix), so no solid-harmonic transform is needed on the device.
// Supported: shells up to g (companions up to h: the classes with a g shell or an h companion run through the runtime
// kernel of eri_generic.hpp).
// The same two contractions by the BASIS parameters of every primitive p (exponent alpha_p, stored coefficient c_p) instead of the
// centres: dqc_eri_grad_basis / dqc_int1e_grad_basis, with d a / d c_p = g_p and d a / d alpha_p = -c_p r_A^2 g_p (an l + 2 shell) as
// per-primitive uncontracted companions.  Orbital shells up to f there (f + 2 = h).
// dqc_eri_grad2 is dqc_eri_grad as the symmetric bilinear form of two matrices, both symmetric or both antisymmetric (the ERI_OUT_GRAD2
// instantiations, compiled in grad2.hip; the two-particle densities of an excited-state Lagrangian).
// Host side: dqc_eri_grad, dqc_eri_grad2, dqc_eri_grad_basis, dqc_df_grad (the same passes over (orbital pair | auxiliary) and (auxiliary |
// auxiliary) for the density-fitted Coulomb energy) and dqc_df_grad3 (those passes against a general three-index density Z[a, b, k]
// and a general G[k, l] -- the ERI_OUT_GRAD3 instantiations; the non-separable part of the RI-MP2 gradient) only parse, build their companions and ordered bra pair lists, name their
// passes (bra list, dirn, gmode, launcher) in a GradJob and say how summed rows become output entries; run_grad_job owns the
// rest -- uploads, the 64 slots of partial sums, the side-stream fork and join, the launches and the host fold.  The two
// one-electron entry points share int1e_grad_setup in the same way.
#include "grad_launch.hpp"

namespace dqc {

// host copy of the solid-harmonic tables (the ones in common.hpp are device symbols)
namespace hostc2s {
#undef C2S_LMAX
#undef C2S_LEN
#define C2S_QUAL static const
#include "cart2sph.inc"
#undef C2S_QUAL
}  // namespace hostc2s

static void cart_offsets(const Basis &b, int nsh, std::vector<int> &cao, int &ncart) {
    cao.resize(nsh);
    ncart = 0;
    for (int i = 0; i < nsh; i++) {
        cao[i] = ncart;
        ncart += (b.shells[i].l + 1) * (b.shells[i].l + 2) / 2;
    }
}

// ordered pairs (first in [f0, f1), second in [0, nsecond)), class index = la * 8 + lb, NO swap
static void build_pairs_ordered(const Basis &b, HostPairs &hp, int f0, int f1, int s0, int s1) {
    std::vector<PairRec> all;
    for (int i = f0; i < f1; i++) {
        const HostShell &A = b.shells[i];
        if (A.l < 0) continue;  // placeholder (no down companion of an s shell)
        for (int j = s0; j < s1; j++) {
            const HostShell &B = b.shells[j];
            PairRec pr;
            pr.a = i; pr.b = j; pr.cls = A.l * 8 + B.l;
            double ab2 = 0;
            for (int d = 0; d < 3; d++) ab2 += (A.r[d] - B.r[d]) * (A.r[d] - B.r[d]);
            for (int ip = 0; ip < A.nprim; ip++)
                for (int jp = 0; jp < B.nprim; jp++) {
                    const double ea = b.exps[A.prim_off + ip], eb = b.exps[B.prim_off + jp], p = ea + eb;
                    const double arg = ea * eb / p * ab2;
                    if (arg > 100.0) continue;
                    if (prim_pair_negligible(b.coefs[A.prim_off + ip] * b.coefs[B.prim_off + jp] * std::exp(-arg) / p, ab2, A.l + B.l)) continue;
                    pr.pp.push_back(p);
                    for (int d = 0; d < 3; d++) pr.pp.push_back((ea * A.r[d] + eb * B.r[d]) / p);
                    pr.pp.push_back(b.coefs[A.prim_off + ip] * b.coefs[B.prim_off + jp] * std::exp(-arg) / p);  // c_a c_b K_ab / p
                }
            all.push_back(std::move(pr));
        }
    }
    pack_pairs(all, hp, 5);
}

// companion shells of the centre derivative, appended to the N shells of the table: [N, 2N) up (l + 1, coefficients 2 alpha c),
// [2N, 3N) down (l - 1; l = -1 marks "none")
static void append_centre_companions(Basis &b, int N) {
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < N; i++) {
            HostShell h = b.shells[i];
            h.l = pass == 0 ? h.l + 1 : h.l - 1;
            const int po = (int)b.exps.size();
            for (int p = 0; p < h.nprim; p++) {
                const double e = b.exps[b.shells[i].prim_off + p], c = b.coefs[b.shells[i].prim_off + p];
                b.exps.push_back(e);
                b.coefs.push_back(pass == 0 ? 2.0 * e * c : c);
            }
            h.prim_off = po;
            b.shells.push_back(h);
        }
}

// density-fitting gradients: ket pairs are (auxiliary shell, unit), classes (LC, 0), LC up to f
template <int LA, int LB, int MODE>
static int launch_grad_bra_df(const GradCtx &c, hipStream_t st) {
    int rc;
#define DQC_GK(LC) \
    if ((rc = launch_grad_class<LA, LB, LC, 0, MODE>(c, st))) return rc;
    DQC_GK(0) DQC_GK(1) DQC_GK(2) DQC_GK(3)
#undef DQC_GK
    return 0;
}

template <int MODE = ERI_OUT_GRAD>
static int launch_grad_df3c(const GradCtx &c, hipStream_t st) {
    int rc;
    if ((rc = launch_grad_generic<MODE>(c, true, DQC_LMAX, st))) return rc;
#define DQC_GB(LA) \
    if ((rc = launch_grad_bra_df<LA, 0, MODE>(c, st)) || (rc = launch_grad_bra_df<LA, 1, MODE>(c, st)) || (rc = launch_grad_bra_df<LA, 2, MODE>(c, st)) || (rc = launch_grad_bra_df<LA, 3, MODE>(c, st))) return rc;
    DQC_GB(0) DQC_GB(1) DQC_GB(2) DQC_GB(3) DQC_GB(4)
#undef DQC_GB
    return 0;
}

template <int MODE = ERI_OUT_GRAD>
static int launch_grad_df2c(const GradCtx &c, hipStream_t st) {
    int rc;
    if ((rc = launch_grad_generic<MODE>(c, true, 0, st))) return rc;
    if ((rc = launch_grad_bra_df<0, 0, MODE>(c, st)) || (rc = launch_grad_bra_df<1, 0, MODE>(c, st)) || (rc = launch_grad_bra_df<2, 0, MODE>(c, st)) ||
        (rc = launch_grad_bra_df<3, 0, MODE>(c, st)) || (rc = launch_grad_bra_df<4, 0, MODE>(c, st)))
        return rc;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// host driver of a GRAD-mode pass set: dqc_eri_grad, dqc_eri_grad_basis and dqc_df_grad describe their work as a GradJob
// ---------------------------------------------------------------------------------------------
struct GradPass {
    const HostPairs *bra;  // ordered pairs (companion shell, original shell): build_pairs_ordered
    int dirn, gmode;       // EriOut::dirn and EriOut::gmode of the pass
    int (*launch)(const GradCtx &, hipStream_t);  // launch_grad_all, launch_grad_df3c or launch_grad_df2c
};

struct GradJob {
    const char *who = nullptr;  // the entry point, for the error strings
    Basis b;                    // the parsed table, then its companion shells
    HostPairs hket;
    std::vector<GradPass> passes;
    std::vector<int> cao, rows;  // per shell below norig: Cartesian offset, row of the partial sums (EriOut::cao, EriOut::sh_atom)
    int ncart = 0, nrow = 0, norig = 0;
    EriOut og{0, 0, 0, 0};  // what only some entry points set: jscale, kscale, ccart
    bool fork = false;      // deal the class launches to the side streams
    int wmap_depth = 0;     // > 0: depth-binned wave map for class pairs at least this deep (GradCtx)
};

// the nuclear forms: the rows are the atoms, g[a][d] += row[a][d]
static void add_rows(const std::vector<double> &row, std::vector<double> &g) {
    for (size_t i = 0; i < g.size(); i++) g[i] += row[i];
}

// Uploads the tables of the job, runs its passes into 64 zeroed slots of (nrow, 3) partial sums, sums the slots on the host and
// lets fold(row, out) add the summed rows to the host copy of d_out (nout doubles), which is then written back.
template <class Fold>
static int run_grad_job(GradJob &j, const double *d_dcart, double *d_out, size_t nout, Fold fold, hipStream_t st) {
    const std::string who(j.who);
    int rc;
    if ((rc = boys_table_ensure())) return rc;
    // upload_shells needs l >= 0 everywhere: placeholders become s shells (never referenced by a pair)
    for (HostShell &h : j.b.shells)
        if (h.l < 0) h.l = 0;
    DevPool pool;       // synchronous: the call ends with a stream synchronise
    DevPool wpool(st);  // stream-ordered, for the wave tables alone
    GradCtx c;
    if (j.wmap_depth > 0) { c.pool = &wpool; c.wmap_depth = j.wmap_depth; }
    if ((rc = upload_shells(c.ds, j.b, pool, st))) { set_error(who + ": device upload failed"); return rc; }
    std::vector<DevPairs> dbra(j.passes.size());
    for (size_t k = 0; k < dbra.size() && !rc; k++) rc = upload_pairs(pool, *j.passes[k].bra, dbra[k], st);
    int *d_cao = nullptr, *d_rows = nullptr;
    if (rc || (rc = upload_pairs(pool, j.hket, c.dket, st)) || (rc = pool.upload(&d_cao, j.cao, st)) ||
        (rc = pool.upload(&d_rows, j.rows, st))) {
        set_error(who + ": device upload failed");
        return rc;
    }
    const int nslot = 64;
    const size_t npart = (size_t)nslot * j.nrow * 3;
    double *d_part = nullptr;
    if (hipMalloc((void **)&d_part, sizeof(double) * npart) != hipSuccess) { set_error(who + ": out of memory"); return DQC_ENOMEM; }
    pool.ptrs.push_back(d_part);
    DQC_HIP(hipMemsetAsync(d_part, 0, sizeof(double) * npart, st));
    c.hket = &j.hket;
    c.og = j.og;
    c.og.dcart = d_dcart; c.og.ncart = j.ncart; c.og.cao = d_cao; c.og.sh_atom = d_rows; c.og.gpart = d_part;
    c.og.nslot = nslot; c.og.natm = j.nrow; c.og.norig = j.norig;
    SideJoin sj;  // (declared after the scratch pools of this call: destroyed, i.e. joined, before they are released)
    if (j.fork) {
        if ((c.side = side_streams()) != nullptr && (rc = c.side->fork(st))) { set_error(who + ": stream fork failed"); return rc; }
        sj.arm(c.side, st);
    }
    for (size_t k = 0; k < dbra.size(); k++) {
        const GradPass &p = j.passes[k];
        c.dbra = dbra[k]; c.hbra = p.bra; c.og.dirn = p.dirn; c.og.gmode = p.gmode;
        if ((rc = p.launch(c, st))) return rc;
    }
    if ((rc = sj.done())) { set_error(who + ": stream join failed"); return rc; }
    // fold the slots into d_out on the host side of the stream: tiny
    std::vector<double> part(npart), row((size_t)j.nrow * 3, 0.0), out(nout);
    DQC_HIP(hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
    DQC_HIP(hipMemcpyAsync(out.data(), d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, st));
    DQC_HIP(hipStreamSynchronize(st));
    for (int sidx = 0; sidx < nslot; sidx++)
        for (size_t i = 0; i < row.size(); i++) row[i] += part[sidx * row.size() + i];
    fold(row, out);
    DQC_HIP(hipMemcpyAsync(d_out, out.data(), sizeof(double) * out.size(), hipMemcpyHostToDevice, st));
    DQC_HIP(hipStreamSynchronize(st));
    return DQC_OK;
}

// ---------------------------------------------------------------------------------------------
// one-electron part: one thread per ORDERED shell pair (a, b), derivative on a's centre
// ---------------------------------------------------------------------------------------------
constexpr int G1 = DQC_LMAX + 2, G3 = DQC_LMAX + 3;  // bra index up to l + 1 (the derivative), ket index up to l + 2 (kinetic)

DQC_DEV void overlap_1d_g(double s[G1][G3], int la, int lb, double PA, double PB, double hp) {
    s[0][0] = 1.0;
    for (int i = 0; i < la; i++) s[i + 1][0] = PA * s[i][0] + (i ? i * hp * s[i - 1][0] : 0.0);
    for (int j = 0; j < lb; j++)
        for (int i = 0; i <= la; i++)
            s[i][j + 1] = PB * s[i][j] + (j ? j * hp * s[i][j - 1] : 0.0) + (i ? i * hp * s[i - 1][j] : 0.0);
}

template <int N>
DQC_DEV void nuc_grad_accumulate(double g3[3], int la, int lb, int nb, double a, double p, const double *P, const double *A,
                                 const double *AB, const double *C, double pref, const double *dblk, size_t nc) {
    // sum_{ca,cb} D[ca][cb] * d/dA (ca | 1/|r - C| | cb), added to g3 (pref carries -Z, coefficients, K, 2 pi / p)
    const double X = p * ((P[0] - C[0]) * (P[0] - C[0]) + (P[1] - C[1]) * (P[1] - C[1]) + (P[2] - C[2]) * (P[2] - C[2]));
    double u[N], w[N];
    rys_roots<N>(X, u, w);
    for (int r = 0; r < N; r++) {
        double g[3][2 * DQC_LMAX + 2][G1];
        const double b10 = 0.5 * (1.0 - u[r]) / p;
        for (int d = 0; d < 3; d++) {
            const double c00 = (P[d] - A[d]) - u[r] * (P[d] - C[d]);
            g[d][0][0] = 1.0;
            g[d][1][0] = c00;
            for (int n = 1; n < la + 1 + lb; n++) g[d][n + 1][0] = c00 * g[d][n][0] + n * b10 * g[d][n - 1][0];
            for (int j = 1; j <= lb; j++)
                for (int i = 0; i <= la + 1 + lb - j; i++) g[d][i][j] = g[d][i + 1][j - 1] + AB[d] * g[d][i][j - 1];
        }
        const double wr = pref * w[r];
        int ca = 0;
        for (int ax = la; ax >= 0; ax--)
            for (int ay = la - ax; ay >= 0; ay--, ca++) {
                const int az = la - ax - ay;
                int cb = 0;
                for (int bx = lb; bx >= 0; bx--)
                    for (int by = lb - bx; by >= 0; by--, cb++) {
                        const int bz = lb - bx - by;
                        const double dd = wr * dblk[ca * nc + cb];
                        const double gx = g[0][ax][bx], gy = g[1][ay][by], gz = g[2][az][bz];
                        const double dgx = 2.0 * a * g[0][ax + 1][bx] - (ax ? ax * g[0][ax - 1][bx] : 0.0);
                        const double dgy = 2.0 * a * g[1][ay + 1][by] - (ay ? ay * g[1][ay - 1][by] : 0.0);
                        const double dgz = 2.0 * a * g[2][az + 1][bz] - (az ? az * g[2][az - 1][bz] : 0.0);
                        g3[0] += dd * dgx * gy * gz;
                        g3[1] += dd * gx * dgy * gz;
                        g3[2] += dd * gx * gy * dgz;
                    }
            }
    }
}

__global__ __launch_bounds__(64) void int1e_grad_kernel(double *__restrict__ grad, DevShells sh, const int *__restrict__ cao,
                                  const int *__restrict__ sh_atom, const double *__restrict__ dcart,
                                  const double *__restrict__ wcart, int ncart, int natm,
                                  const double *__restrict__ atom_xyz, const double *__restrict__ atom_z) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= sh.nsh * sh.nsh) return;
    const int ish = pair / sh.nsh, jsh = pair % sh.nsh;
    const int la = sh.l[ish], lb = sh.l[jsh];
    const int nb = (lb + 1) * (lb + 2) / 2;
    const size_t nc = ncart;
    const double A[3] = {sh.xyz[ish * 3], sh.xyz[ish * 3 + 1], sh.xyz[ish * 3 + 2]};
    const double B[3] = {sh.xyz[jsh * 3], sh.xyz[jsh * 3 + 1], sh.xyz[jsh * 3 + 2]};
    const double AB[3] = {A[0] - B[0], A[1] - B[1], A[2] - B[2]};
    const double ab2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
    const double *dblk = dcart + (size_t)cao[ish] * nc + cao[jsh];
    const double *wblk = wcart + (size_t)cao[ish] * nc + cao[jsh];
    double ga[3] = {0.0, 0.0, 0.0};  // basis-centre terms, go to a's atom
    const bool one_nuc = (int)gridDim.y >= natm;
    double gn[3] = {0.0, 0.0, 0.0};  // operator-derivative term of this thread's nucleus (one_nuc)
    for (int ip = 0; ip < sh.nprim[ish]; ip++)
        for (int jp = 0; jp < sh.nprim[jsh]; jp++) {
            const double a = sh.exps[sh.prim_off[ish] + ip], b = sh.exps[sh.prim_off[jsh] + jp];
            const double cc = sh.coefs[sh.prim_off[ish] + ip] * sh.coefs[sh.prim_off[jsh] + jp];
            const double p = a + b, hp = 0.5 / p;
            const double K = exp(-a * b / p * ab2);
            double P[3];
            for (int d = 0; d < 3; d++) P[d] = (a * A[d] + b * B[d]) / p;
            // ---- overlap and kinetic
            double s[3][G1][G3];
            for (int d = 0; d < 3; d++) overlap_1d_g(s[d], la + 1, lb + 2, P[d] - A[d], P[d] - B[d], hp);
            const double pref = cc * K * pow(M_PI / p, 1.5);
            auto tt = [&](int d, int i, int j) {  // -1/2 d2/dx2 on the ket index, 1D
                return -2.0 * b * b * s[d][i][j + 2] + b * (2 * j + 1) * s[d][i][j] - (j >= 2 ? 0.5 * j * (j - 1) * s[d][i][j - 2] : 0.0);
            };
            int ca = 0;
            // (the launch is split over the nuclei along grid.y -- one thread per shell pair walked all primitive pairs and all
            // nuclei alone: 9 ms for a 20-atom molecule on 144 waves; the overlap / kinetic part belongs to split 0)
            for (int ax = (blockIdx.y == 0 ? la : -1); ax >= 0; ax--)
                for (int ay = la - ax; ay >= 0; ay--, ca++) {
                    const int az = la - ax - ay;
                    const int av[3] = {ax, ay, az};
                    int cb = 0;
                    for (int bx = lb; bx >= 0; bx--)
                        for (int by = lb - bx; by >= 0; by--, cb++) {
                            const int bz = lb - bx - by;
                            const int bv[3] = {bx, by, bz};
                            double sv[3], tv[3], dsv[3], dtv[3];
                            for (int d = 0; d < 3; d++) {
                                sv[d] = s[d][av[d]][bv[d]];
                                tv[d] = tt(d, av[d], bv[d]);
                                dsv[d] = 2.0 * a * s[d][av[d] + 1][bv[d]] - (av[d] ? av[d] * s[d][av[d] - 1][bv[d]] : 0.0);
                                dtv[d] = 2.0 * a * tt(d, av[d] + 1, bv[d]) - (av[d] ? av[d] * tt(d, av[d] - 1, bv[d]) : 0.0);
                            }
                            const double dd = pref * dblk[ca * nc + cb], ww = pref * wblk[ca * nc + cb];
                            for (int d = 0; d < 3; d++) {
                                const int e = (d + 1) % 3, f = (d + 2) % 3;
                                const double dS = dsv[d] * sv[e] * sv[f];
                                const double dT = dtv[d] * sv[e] * sv[f] + dsv[d] * tv[e] * sv[f] + dsv[d] * sv[e] * tv[f];
                                ga[d] += dd * dT - ww * dS;
                            }
                        }
                }
            // ---- nuclear attraction, nucleus by nucleus (operator derivative by translational invariance)
            const int nroots = (la + 1 + lb) / 2 + 1;
            for (int ic = blockIdx.y; ic < natm; ic += gridDim.y) {
                const double prn = -atom_z[ic] * cc * K * 2.0 * M_PI / p;
                const double *C = atom_xyz + ic * 3;
                double g3[3] = {0.0, 0.0, 0.0};
                switch (nroots) {
                case 1: nuc_grad_accumulate<1>(g3, la, lb, nb, a, p, P, A, AB, C, prn, dblk, nc); break;
                case 2: nuc_grad_accumulate<2>(g3, la, lb, nb, a, p, P, A, AB, C, prn, dblk, nc); break;
                case 3: nuc_grad_accumulate<3>(g3, la, lb, nb, a, p, P, A, AB, C, prn, dblk, nc); break;
                case 4: nuc_grad_accumulate<4>(g3, la, lb, nb, a, p, P, A, AB, C, prn, dblk, nc); break;
                default: nuc_grad_accumulate<5>(g3, la, lb, nb, a, p, P, A, AB, C, prn, dblk, nc); break;
                }
                for (int d = 0; d < 3; d++) {
                    ga[d] += g3[d];
                    // (one nucleus per thread when the launch has a y-slice per nucleus: its operator-derivative term is summed over
                    // the primitive pairs and added once -- 35 M atomics on 60 addresses were most of this kernel's time)
                    if (one_nuc) gn[d] += g3[d];
                    else atomicAdd(&grad[ic * 3 + d], -2.0 * g3[d]);
                }
            }
        }
    for (int d = 0; d < 3; d++) atomicAdd(&grad[sh_atom[ish] * 3 + d], 2.0 * ga[d]);
    if (one_nuc)
        for (int d = 0; d < 3; d++) atomicAdd(&grad[blockIdx.y * 3 + d], -2.0 * gn[d]);
}

// ---------------------------------------------------------------------------------------------
// basis-parameter derivatives, one-electron part: one thread per ORDERED shell pair (a, b), derivative on a's primitives.
// d a / d c_p = g_p (the primitive alone), d a / d alpha_p = -c_p r_A^2 g_p = -c_p sum_d g_p[power of d raised by 2]: the same
// 1-D tables as int1e_grad_kernel with the bra index reaching l + 2.  Orbital shells up to f (the host refuses more).
// ---------------------------------------------------------------------------------------------
static_assert(G1 >= GRAD_LMAX + 3 && G3 >= GRAD_LMAX + 3, "1-D overlap tables: bra index l + 2, ket index l + 2 for f shells");

template <int N>
DQC_DEV void nuc_basis_accumulate(double &vc, double &va, int la, int lb, double p, const double *P, const double *A,
                                  const double *AB, const double *C, double pref, const double *dblk, size_t nc) {
    // vc += pref sum_{ca,cb} D[ca][cb] (ca | 1/|r - C| | cb),  va += the same with r_A^2 ca in the bra (pref carries -Z, c_b, K, 2 pi / p)
    const double X = p * ((P[0] - C[0]) * (P[0] - C[0]) + (P[1] - C[1]) * (P[1] - C[1]) + (P[2] - C[2]) * (P[2] - C[2]));
    double u[N], w[N];
    rys_roots<N>(X, u, w);
    for (int r = 0; r < N; r++) {
        double g[3][2 * DQC_LMAX + 2][G1];  // first index up to la + 2 + lb <= 2 GRAD_LMAX + 2
        const double b10 = 0.5 * (1.0 - u[r]) / p;
        for (int d = 0; d < 3; d++) {
            const double c00 = (P[d] - A[d]) - u[r] * (P[d] - C[d]);
            g[d][0][0] = 1.0;
            g[d][1][0] = c00;
            for (int n = 1; n < la + 2 + lb; n++) g[d][n + 1][0] = c00 * g[d][n][0] + n * b10 * g[d][n - 1][0];
            for (int j = 1; j <= lb; j++)
                for (int i = 0; i <= la + 2 + lb - j; i++) g[d][i][j] = g[d][i + 1][j - 1] + AB[d] * g[d][i][j - 1];
        }
        double s0 = 0.0, s2 = 0.0;
        int ca = 0;
        for (int ax = la; ax >= 0; ax--)
            for (int ay = la - ax; ay >= 0; ay--, ca++) {
                const int az = la - ax - ay;
                int cb = 0;
                for (int bx = lb; bx >= 0; bx--)
                    for (int by = lb - bx; by >= 0; by--, cb++) {
                        const int bz = lb - bx - by;
                        const double dd = dblk[ca * nc + cb];
                        const double gx = g[0][ax][bx], gy = g[1][ay][by], gz = g[2][az][bz];
                        s0 += dd * gx * gy * gz;
                        s2 += dd * (g[0][ax + 2][bx] * gy * gz + gx * g[1][ay + 2][by] * gz + gx * gy * g[2][az + 2][bz]);
                    }
            }
        vc += pref * w[r] * s0;
        va += pref * w[r] * s2;
    }
}

__global__ __launch_bounds__(64) void int1e_grad_basis_kernel(double *__restrict__ out, DevShells sh, const int *__restrict__ cao,
                                  const double *__restrict__ dcart, const double *__restrict__ wcart, int ncart, int natm,
                                  const double *__restrict__ atom_xyz, const double *__restrict__ atom_z) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= sh.nsh * sh.nsh) return;
    const int ish = pair / sh.nsh, jsh = pair % sh.nsh;
    const int la = sh.l[ish], lb = sh.l[jsh];
    const size_t nc = ncart;
    const double A[3] = {sh.xyz[ish * 3], sh.xyz[ish * 3 + 1], sh.xyz[ish * 3 + 2]};
    const double B[3] = {sh.xyz[jsh * 3], sh.xyz[jsh * 3 + 1], sh.xyz[jsh * 3 + 2]};
    const double AB[3] = {A[0] - B[0], A[1] - B[1], A[2] - B[2]};
    const double ab2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
    const double *dblk = dcart + (size_t)cao[ish] * nc + cao[jsh];
    const double *wblk = wcart + (size_t)cao[ish] * nc + cao[jsh];
    const int nroots = (la + 2 + lb) / 2 + 1;
    for (int ip = 0; ip < sh.nprim[ish]; ip++) {
        const double a = sh.exps[sh.prim_off[ish] + ip];
        double vc = 0.0, va = 0.0;  // sum_b [D (g_p|T + V|b) - W (g_p|b)] and the same with r_A^2 g_p
        for (int jp = 0; jp < sh.nprim[jsh]; jp++) {
            const double b = sh.exps[sh.prim_off[jsh] + jp];
            const double p = a + b, hp = 0.5 / p;
            const double cK = sh.coefs[sh.prim_off[jsh] + jp] * exp(-a * b / p * ab2);
            double P[3];
            for (int d = 0; d < 3; d++) P[d] = (a * A[d] + b * B[d]) / p;
            if (blockIdx.y == 0) {  // ---- overlap and kinetic (the nuclei are split over grid.y as in int1e_grad_kernel)
                double s[3][G1][G3];
                for (int d = 0; d < 3; d++) overlap_1d_g(s[d], la + 2, lb + 2, P[d] - A[d], P[d] - B[d], hp);
                const double pref = cK * pow(M_PI / p, 1.5);
                auto tt = [&](int d, int i, int j) {  // -1/2 d2/dx2 on the ket index, 1D
                    return -2.0 * b * b * s[d][i][j + 2] + b * (2 * j + 1) * s[d][i][j] - (j >= 2 ? 0.5 * j * (j - 1) * s[d][i][j - 2] : 0.0);
                };
                int ca = 0;
                for (int ax = la; ax >= 0; ax--)
                    for (int ay = la - ax; ay >= 0; ay--, ca++) {
                        const int av[3] = {ax, ay, la - ax - ay};
                        int cb = 0;
                        for (int bx = lb; bx >= 0; bx--)
                            for (int by = lb - bx; by >= 0; by--, cb++) {
                                const int bv[3] = {bx, by, lb - bx - by};
                                double sv[3], tv[3], s2[3], t2[3];
                                for (int d = 0; d < 3; d++) {
                                    sv[d] = s[d][av[d]][bv[d]];
                                    tv[d] = tt(d, av[d], bv[d]);
                                    s2[d] = s[d][av[d] + 2][bv[d]];
                                    t2[d] = tt(d, av[d] + 2, bv[d]);
                                }
                                const double S0 = sv[0] * sv[1] * sv[2];
                                const double T0 = tv[0] * sv[1] * sv[2] + sv[0] * tv[1] * sv[2] + sv[0] * sv[1] * tv[2];
                                double S2 = 0.0, T2 = 0.0;
                                for (int d = 0; d < 3; d++) {
                                    const int e = (d + 1) % 3, f = (d + 2) % 3;
                                    S2 += s2[d] * sv[e] * sv[f];
                                    T2 += t2[d] * sv[e] * sv[f] + s2[d] * (tv[e] * sv[f] + sv[e] * tv[f]);
                                }
                                const double dd = pref * dblk[ca * nc + cb], ww = pref * wblk[ca * nc + cb];
                                vc += dd * T0 - ww * S0;
                                va += dd * T2 - ww * S2;
                            }
                    }
            }
            // ---- nuclear attraction, nucleus by nucleus
            for (int ic = blockIdx.y; ic < natm; ic += gridDim.y) {
                const double prn = -atom_z[ic] * cK * 2.0 * M_PI / p;
                const double *C = atom_xyz + ic * 3;
                switch (nroots) {
                case 2: nuc_basis_accumulate<2>(vc, va, la, lb, p, P, A, AB, C, prn, dblk, nc); break;
                case 3: nuc_basis_accumulate<3>(vc, va, la, lb, p, P, A, AB, C, prn, dblk, nc); break;
                case 4: nuc_basis_accumulate<4>(vc, va, la, lb, p, P, A, AB, C, prn, dblk, nc); break;
                default: nuc_basis_accumulate<5>(vc, va, la, lb, p, P, A, AB, C, prn, dblk, nc); break;
                }
            }
        }
        const size_t row = sh.prim_off[ish] + ip;  // (the primitives of the table in shell order: parse_basis)
        atomicAdd(&out[row * 2], -2.0 * sh.coefs[row] * va);
        atomicAdd(&out[row * 2 + 1], 2.0 * vc);
    }
}

// ---------------------------------------------------------------------------------------------
// electronic electrostatic potential at points: V_C = sum_ab D_ab <a| 1/|r - P_C| |b>  (the alchemical derivative
// dE/dZ_C = -V_C + ...; the Rys quadrature of the nuclear attraction, contracted with D on the fly)
// ---------------------------------------------------------------------------------------------
constexpr int PL1 = DQC_LMAX + 1;

template <int N>
DQC_DEV double nuc_pot_accumulate(int la, int lb, double p, const double *P, const double *A, const double *AB, const double *C,
                                  const double *dab, const double *dba, size_t nc) {
    // sum_{ca,cb} (D[ca][cb] + D^T[ca][cb]) (ca | 1/|r - C| | cb) / (pref) -- dba == nullptr on a diagonal shell pair
    const double X = p * ((P[0] - C[0]) * (P[0] - C[0]) + (P[1] - C[1]) * (P[1] - C[1]) + (P[2] - C[2]) * (P[2] - C[2]));
    double u[N], w[N];
    rys_roots<N>(X, u, w);
    double acc = 0.0;
    for (int r = 0; r < N; r++) {
        double g[3][2 * DQC_LMAX + 1][PL1];
        const double b10 = 0.5 * (1.0 - u[r]) / p;
        for (int d = 0; d < 3; d++) {
            const double c00 = (P[d] - A[d]) - u[r] * (P[d] - C[d]);
            g[d][0][0] = 1.0;
            if (la + lb > 0) g[d][1][0] = c00;
            for (int n = 1; n < la + lb; n++) g[d][n + 1][0] = c00 * g[d][n][0] + n * b10 * g[d][n - 1][0];
            for (int j = 1; j <= lb; j++)
                for (int i = 0; i <= la + lb - j; i++) g[d][i][j] = g[d][i + 1][j - 1] + AB[d] * g[d][i][j - 1];
        }
        double sr = 0.0;
        int ca = 0;
        for (int ax = la; ax >= 0; ax--)
            for (int ay = la - ax; ay >= 0; ay--, ca++) {
                const int az = la - ax - ay;
                int cb = 0;
                for (int bx = lb; bx >= 0; bx--)
                    for (int by = lb - bx; by >= 0; by--, cb++) {
                        const int bz = lb - bx - by;
                        const double dd = dab[ca * nc + cb] + (dba != nullptr ? dba[cb * nc + ca] : 0.0);
                        sr += dd * g[0][ax][bx] * g[1][ay][by] * g[2][az][bz];
                    }
            }
        acc += w[r] * sr;
    }
    return acc;
}

// One thread per unordered shell pair (a >= b), 256 pairs per block; the points are split over grid.y (a block walks the points
// blockIdx.y, blockIdx.y + gridDim.y, ...).  Per point the block's threads are summed in a fixed order (wave butterfly, then
// the four wave sums in order) and the block's partial is STORED to part[point][blockIdx.x]: no atomics, and the second pass
// (int1e_potential_sum) adds the partials of a point in block order, so the result is bit-reproducible.
constexpr int POT_BLOCK = 256;
__global__ __launch_bounds__(POT_BLOCK) void int1e_potential_kernel(double *__restrict__ part, DevShells sh, const int *__restrict__ cao,
                                                                    const double *__restrict__ dcart, int ncart,
                                                                    const double *__restrict__ pts, int npts) {
    __shared__ double swave[POT_BLOCK / 64];
    const long long npair = (long long)sh.nsh * (sh.nsh + 1) / 2;
    const long long q = (long long)blockIdx.x * POT_BLOCK + threadIdx.x;
    const bool live = q < npair;
    int ish = 0, jsh = 0;
    if (live) {
        ish = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
        while ((long long)ish * (ish + 1) / 2 > q) ish--;
        while ((long long)(ish + 1) * (ish + 2) / 2 <= q) ish++;
        jsh = (int)(q - (long long)ish * (ish + 1) / 2);
    }
    const int la = sh.l[ish], lb = sh.l[jsh];
    const size_t nc = ncart;
    const double A[3] = {sh.xyz[ish * 3], sh.xyz[ish * 3 + 1], sh.xyz[ish * 3 + 2]};
    const double B[3] = {sh.xyz[jsh * 3], sh.xyz[jsh * 3 + 1], sh.xyz[jsh * 3 + 2]};
    const double AB[3] = {A[0] - B[0], A[1] - B[1], A[2] - B[2]};
    const double ab2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
    const double *dab = dcart + (size_t)cao[ish] * nc + cao[jsh];
    const double *dba = ish != jsh ? dcart + (size_t)cao[jsh] * nc + cao[ish] : nullptr;  // (V is symmetric: D_ab + D_ba)
    const int nroots = (la + lb) / 2 + 1;
    for (int ic = blockIdx.y; ic < npts; ic += gridDim.y) {
        const double C[3] = {pts[ic * 3], pts[ic * 3 + 1], pts[ic * 3 + 2]};
        double v = 0.0;
        if (live) {
            for (int ip = 0; ip < sh.nprim[ish]; ip++)
                for (int jp = 0; jp < sh.nprim[jsh]; jp++) {
                    const double a = sh.exps[sh.prim_off[ish] + ip], b = sh.exps[sh.prim_off[jsh] + jp];
                    const double cc = sh.coefs[sh.prim_off[ish] + ip] * sh.coefs[sh.prim_off[jsh] + jp];
                    const double p = a + b;
                    const double pref = cc * exp(-a * b / p * ab2) * 2.0 * M_PI / p;
                    double P[3];
                    for (int d = 0; d < 3; d++) P[d] = (a * A[d] + b * B[d]) / p;
                    double s;
                    switch (nroots) {
                    case 1: s = nuc_pot_accumulate<1>(la, lb, p, P, A, AB, C, dab, dba, nc); break;
                    case 2: s = nuc_pot_accumulate<2>(la, lb, p, P, A, AB, C, dab, dba, nc); break;
                    case 3: s = nuc_pot_accumulate<3>(la, lb, p, P, A, AB, C, dab, dba, nc); break;
                    case 4: s = nuc_pot_accumulate<4>(la, lb, p, P, A, AB, C, dab, dba, nc); break;
                    default: s = nuc_pot_accumulate<5>(la, lb, p, P, A, AB, C, dab, dba, nc); break;
                    }
                    v += pref * s;
                }
        }
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) swave[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int wv = 0; wv < POT_BLOCK / 64; wv++) t += swave[wv];
            part[(size_t)ic * gridDim.x + blockIdx.x] = t;
        }
        __syncthreads();  // (swave is rewritten for the next point)
    }
}

__global__ __launch_bounds__(64) void int1e_potential_sum(double *__restrict__ out, const double *__restrict__ part, int nblk, int npts) {
    const int ic = blockIdx.x * blockDim.x + threadIdx.x;
    if (ic >= npts) return;
    double t = 0.0;
    for (int k = 0; k < nblk; k++) t += part[(size_t)ic * nblk + k];
    out[ic] = t;
}

// orbital shells up to f: the alpha derivative needs the l + 2 shell, and h is the highest the Rys kernels reach
static int basis_grad_lcheck(const Basis &b, const char *who) {
    for (const HostShell &h : b.shells)
        if (h.l > GRAD_LMAX) {
            set_error((std::string(who) + ": basis-parameter derivatives support orbital shells up to f (a g shell needs l + 2 = i integrals)").c_str());
            return DQC_EINVAL;
        }
    return 0;
}

// what dqc_int1e_grad and dqc_int1e_grad_basis (`basis`: with its refusal of shells above f) set up alike: the table parsed with the
// charges `zs`, its Cartesian offsets, the device copies, and the launch grid (64 ordered shell pairs per block, the nuclei along y)
struct Int1eGradSetup {
    Basis b;
    std::vector<int> cao;
    int ncart = 0;
    DevPool pool;
    DevShells ds;
    double *d_xyz = nullptr, *d_z = nullptr;
    int *d_cao = nullptr;
    dim3 grid;
};
// nbas == 0: returns DQC_OK with nothing uploaded (the callers return, too)
static int int1e_grad_setup(Int1eGradSetup &s, const char *who, bool basis, const int *atm, int natm, const int *bas, int nbas,
                            const double *env, int nenv, const double *zs, hipStream_t st) {
    int rc = parse_basis(s.b, atm, natm, bas, nbas, env, nenv, zs);
    if (rc) return rc;
    if (nbas == 0) return DQC_OK;
    if (basis && (rc = basis_grad_lcheck(s.b, who))) return rc;
    cart_offsets(s.b, nbas, s.cao, s.ncart);
    if ((rc = upload_shells(s.ds, s.b, s.pool, st)) || (rc = s.pool.upload(&s.d_xyz, s.b.atom_xyz, st)) ||
        (rc = s.pool.upload(&s.d_z, s.b.atom_z, st)) || (rc = s.pool.upload(&s.d_cao, s.cao, st))) {
        set_error(std::string(who) + ": device upload failed");
        return rc;
    }
    const int npair = nbas * nbas;
    s.grid = dim3((npair + 63) / 64, natm < 32 ? natm : 32);
    return DQC_OK;
}

}  // namespace dqc

extern "C" {

int dqc_ncart(const int *bas, int nbas) {
    int n = 0;
    for (int i = 0; i < nbas; i++) n += (bas[i * 8 + 1] + 1) * (bas[i * 8 + 1] + 2) / 2;
    return n;
}

int dqc_cart2sph_matrix(double *h_out, const int *bas, int nbas) {
    // HOST array (nao, ncart), block diagonal: chi_m = sum_c T[m][c] g_c for every shell
    using namespace dqc;
    int nao = 0, ncart = dqc_ncart(bas, nbas);
    for (int i = 0; i < nbas; i++) nao += 2 * bas[i * 8 + 1] + 1;
    for (size_t i = 0; i < (size_t)nao * ncart; i++) h_out[i] = 0.0;
    int ao = 0, co = 0;
    for (int i = 0; i < nbas; i++) {
        const int l = bas[i * 8 + 1];
        if (l > C2S_LMAX) { set_error("dqc_cart2sph_matrix: angular momentum above g"); return DQC_EINVAL; }
        const int ns = 2 * l + 1, ncl = (l + 1) * (l + 2) / 2;
        for (int m = 0; m < ns; m++)
            for (int c = 0; c < ncl; c++) h_out[(size_t)(ao + m) * ncart + co + c] = hostc2s::C2S[hostc2s::C2S_OFF[l] + m * ncl + c];
        ao += ns;
        co += ncl;
    }
    return DQC_OK;
}

int dqc_eri_grad(double *d_grad, const double *d_dcart, double jscale, double kscale, const int *atm, int natm, const int *bas, int nbas,
                 const double *env, int nenv, void *stream) {
    // d_grad (natm, 3) += sum_{a in A} sum_bcd (d_A a b|c d) [2 jscale D_ab D_cd - kscale D_ac D_bd]; d_dcart (ncart, ncart)
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    GradJob j;
    j.who = "dqc_eri_grad";
    Basis &b = j.b;
    int rc = parse_basis(b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    if (nbas == 0) return DQC_OK;
    const int N = nbas;
    cart_offsets(b, N, j.cao, j.ncart);
    j.rows.resize(N);
    for (int i = 0; i < N; i++) j.rows[i] = b.shells[i].atom;
    append_centre_companions(b, N);
    HostPairs hup, hdown;
    build_pairs_ordered(b, hup, N, 2 * N, 0, N);
    build_pairs_ordered(b, hdown, 2 * N, 3 * N, 0, N);
    build_pairs(b, j.hket, 0, N);
    j.passes = {{&hup, +1, 0, launch_grad_all<>}, {&hdown, -1, 0, launch_grad_all<>}};
    j.nrow = natm; j.norig = N; j.og.jscale = jscale; j.og.kscale = kscale;
    j.fork = true;
    // the depth-binned wave map of the fill (eri_core.hpp) is OFF here: measured on a 20-atom cc-pVDZ gradient it is slower for every
    // depth threshold -- 0.160 s (classes deeper than 64 primitive quartets), 0.149 (256), 0.140 (1024) against 0.107 s for the flat
    // task maps (DQC_GRAD_WMAP = the depth threshold for A/B runs, 0 / unset = never)
    static const int wmap_env = [] { const char *e = getenv("DQC_GRAD_WMAP"); return e ? atoi(e) : 0; }();
    j.wmap_depth = wmap_env;
    return run_grad_job(j, d_dcart, d_grad, (size_t)natm * 3, add_rows, st);
}

int dqc_eri_grad2(double *d_grad, const double *d_acart, const double *d_bcart, int ncart, int parity_a, int parity_b, double jscale,
                  double kscale, const int *atm, int natm, const int *bas, int nbas, const double *env, int nenv, void *stream) {
    // the symmetric bilinear form whose diagonal is dqc_eri_grad (A = B = D):
    //   d_grad (natm, 3) += sum_{a in A} sum_bcd (d_A a b|c d) [jscale (A_ab B_cd + B_ab A_cd) - kscale / 2 (A_ac B_bd + B_ac A_bd)]
    // d_acart, d_bcart (ncart, ncart); parity_a, parity_b: +1 for an exactly symmetric matrix, -1 for an exactly antisymmetric one,
    // as the caller has verified them (the matrices are device memory).  Only for a same-parity pair is "derivative on the first
    // index" a quarter of the derivative of sum (ab|cd) Gamma_abcd, so every other pair is refused, as is an antisymmetric one with a
    // Coulomb part (A_ab B_cd summed with (ab| symmetric is zero: a non-zero jscale is a mistake of the caller).
    // The ERI_OUT_GRAD2 instantiations (grad2.hip); B rides in EriOut::ccart, which gmode 0 does not read otherwise.
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    GradJob j;
    j.who = "dqc_eri_grad2";
    Basis &b = j.b;
    int rc = parse_basis(b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    const int N = nbas;
    cart_offsets(b, N, j.cao, j.ncart);
    if (ncart != j.ncart) {
        set_error("dqc_eri_grad2: the matrices are (" + std::to_string(ncart) + ", " + std::to_string(ncart) + "), the table has " +
                  std::to_string(j.ncart) + " Cartesian functions");
        return DQC_EINVAL;
    }
    if ((parity_a != 1 && parity_a != -1) || (parity_b != 1 && parity_b != -1)) {
        set_error("dqc_eri_grad2: a parity is +1 (symmetric) or -1 (antisymmetric)");
        return DQC_EINVAL;
    }
    if (parity_a != parity_b) {
        set_error("dqc_eri_grad2: one matrix is symmetric and the other antisymmetric (the bilinear form needs a same-parity pair)");
        return DQC_EINVAL;
    }
    if (parity_a == -1 && jscale != 0.0) {
        set_error("dqc_eri_grad2: an antisymmetric pair has no Coulomb part (jscale must be 0)");
        return DQC_EINVAL;
    }
    if (nbas == 0) return DQC_OK;
    if (d_grad == nullptr || d_acart == nullptr || d_bcart == nullptr) { set_error("dqc_eri_grad2: null pointer"); return DQC_EINVAL; }
    j.rows.resize(N);
    for (int i = 0; i < N; i++) j.rows[i] = b.shells[i].atom;
    append_centre_companions(b, N);
    HostPairs hup, hdown;
    build_pairs_ordered(b, hup, N, 2 * N, 0, N);
    build_pairs_ordered(b, hdown, 2 * N, 3 * N, 0, N);
    build_pairs(b, j.hket, 0, N);
    j.passes = {{&hup, +1, 0, launch_grad2_all}, {&hdown, -1, 0, launch_grad2_all}};
    j.nrow = natm; j.norig = N; j.og.jscale = jscale; j.og.kscale = kscale; j.og.ccart = d_bcart;
    j.fork = true;
    return run_grad_job(j, d_acart, d_grad, (size_t)natm * 3, add_rows, st);
}

int dqc_int1e_grad(double *d_grad, const double *d_dcart, const double *d_wcart, const int *atm, int natm, const int *bas,
                   int nbas, const double *env, int nenv, const double *zs, void *stream) {
    // d_grad (natm, 3) += 2 sum_{a in A} sum_b [D_ab (d_A a|T + V|b) - W_ab (d_A a|b)]  and the Hellmann-Feynman
    // term of every nucleus; d_dcart / d_wcart: Cartesian-basis density and energy-weighted density (ncart, ncart)
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    Int1eGradSetup s;
    int rc = int1e_grad_setup(s, "dqc_int1e_grad", false, atm, natm, bas, nbas, env, nenv, zs, st);
    if (rc || nbas == 0) return rc;
    std::vector<int> sh_atom(nbas);
    for (int i = 0; i < nbas; i++) sh_atom[i] = s.b.shells[i].atom;
    int *d_atom = nullptr;
    if ((rc = s.pool.upload(&d_atom, sh_atom, st))) { set_error("dqc_int1e_grad: device upload failed"); return rc; }
    hipLaunchKernelGGL(int1e_grad_kernel, s.grid, dim3(64), 0, st, d_grad, s.ds, s.d_cao, d_atom, d_dcart, d_wcart, s.ncart, natm, s.d_xyz,
                       s.d_z);
    DQC_CHECK_LAUNCH();
    DQC_HIP(hipStreamSynchronize(st));
    return DQC_OK;
}

int dqc_eri_grad_basis(double *d_out, const double *d_dcart, double jscale, double kscale, const int *atm, int natm, const int *bas,
                       int nbas, const double *env, int nenv, void *stream) {
    // d_out (nprim_total, 2) += sum_{a has p} sum_bcd (d_theta a b|c d) [2 jscale D_ab D_cd - kscale D_ac D_bd], theta = alpha_p
    // (column 0) or c_p (column 1) of every primitive p in table order; d_dcart (ncart, ncart)
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    GradJob j;
    j.who = "dqc_eri_grad_basis";
    Basis &b = j.b;
    int rc = parse_basis(b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    if (nbas == 0) return DQC_OK;
    if ((rc = basis_grad_lcheck(b, j.who))) return rc;
    const int N = nbas, P = (int)b.exps.size();
    std::vector<int> &cao = j.cao, &rows = j.rows;
    cart_offsets(b, N, cao, j.ncart);
    cao.resize(N + 2 * P);
    rows.assign(N + 2 * P, 0);
    // per-primitive companion shells, uncontracted: [N, N + P) the primitive itself (l, coefficient 1),
    // [N + P, N + 2P) its r_A^2 multiple (l + 2, coefficient -c_p).  The GRAD epilogue (eri_core.hpp, dirn 0 / 2) looks both maps up
    // by the companion shell itself: cao = the Cartesian offset of its original shell, rows = its row of the partial sums
    // (2P rows of 3 "directions": row p the same sum three times, row P + p the three raised powers)
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < N; i++)
            for (int p = 0; p < b.shells[i].nprim; p++) {
                HostShell h = b.shells[i];
                const int row = b.shells[i].prim_off + p, comp = N + pass * P + row;
                cao[comp] = cao[i];
                rows[comp] = pass * P + row;
                h.l += 2 * pass;
                h.nprim = 1;
                h.prim_off = (int)b.exps.size();
                b.exps.push_back(b.exps[row]);
                b.coefs.push_back(pass == 0 ? 1.0 : -b.coefs[row]);
                b.shells.push_back(h);
            }
    HostPairs hsame, hup2;
    build_pairs_ordered(b, hsame, N, N + P, 0, N);
    build_pairs_ordered(b, hup2, N + P, N + 2 * P, 0, N);
    build_pairs(b, j.hket, 0, N);
    j.passes = {{&hsame, 0, 0, launch_grad_all<>}, {&hup2, 2, 0, launch_grad_all<>}};
    j.nrow = 2 * P; j.norig = N + 2 * P; j.og.jscale = jscale; j.og.kscale = kscale;
    j.fork = true;
    // alpha_p: the three raised powers of row P + p together; c_p: row p holds the same sum three times
    auto fold = [P](const std::vector<double> &row, std::vector<double> &out) {
        for (int p = 0; p < P; p++) {
            const double *same = &row[(size_t)p * 3], *up2 = &row[(size_t)(P + p) * 3];
            out[(size_t)p * 2] += up2[0] + up2[1] + up2[2];
            out[(size_t)p * 2 + 1] += same[0];
        }
    };
    return run_grad_job(j, d_dcart, d_out, (size_t)P * 2, fold, st);
}

int dqc_int1e_grad_basis(double *d_out, const double *d_dcart, const double *d_wcart, const int *atm, int natm, const int *bas,
                         int nbas, const double *env, int nenv, const double *zs, void *stream) {
    // d_out (nprim_total, 2) += 2 sum_{a has p} sum_b [D_ab (d_theta a|T + V|b) - W_ab (d_theta a|b)], theta = alpha_p (column 0) or
    // c_p (column 1); d_dcart / d_wcart: Cartesian-basis density and energy-weighted density (ncart, ncart)
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    Int1eGradSetup s;
    int rc = int1e_grad_setup(s, "dqc_int1e_grad_basis", true, atm, natm, bas, nbas, env, nenv, zs, st);
    if (rc || nbas == 0) return rc;
    hipLaunchKernelGGL(int1e_grad_basis_kernel, s.grid, dim3(64), 0, st, d_out, s.ds, s.d_cao, d_dcart, d_wcart, s.ncart, natm, s.d_xyz,
                       s.d_z);
    DQC_CHECK_LAUNCH();
    DQC_HIP(hipStreamSynchronize(st));
    return DQC_OK;
}

int dqc_int1e_potential(double *d_out, const double *d_dcart, const double *d_points, int npts, const int *atm, int natm,
                        const int *bas, int nbas, const double *env, int nenv, void *stream) {
    // d_out[C] = sum_ab D_ab <a| 1/|r - P_C| |b>, C < npts; d_dcart (ncart, ncart) Cartesian-basis density, d_points (npts, 3)
    // device coordinates.  Stream-ordered: this call only enqueues.
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    if (npts < 0) { set_error("dqc_int1e_potential: npts must be >= 0"); return DQC_EINVAL; }
    Basis b;
    int rc = parse_basis(b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    if (npts == 0) return DQC_OK;
    if (nbas == 0) {
        DQC_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * npts, st));
        return DQC_OK;
    }
    std::vector<int> cao;
    int ncart;
    cart_offsets(b, nbas, cao, ncart);
    DevPool pool(st);
    DevShells ds;
    int *d_cao = nullptr;
    if ((rc = upload_shells(ds, b, pool, st)) || (rc = pool.upload(&d_cao, cao, st))) {
        set_error("dqc_int1e_potential: device upload failed");
        return rc;
    }
    const long long npair = (long long)nbas * (nbas + 1) / 2;
    const long long nblk = (npair + POT_BLOCK - 1) / POT_BLOCK;
    const int ny = npts < 65535 ? npts : 65535;
    double *d_part = nullptr;
    if ((rc = pool.alloc(&d_part, (size_t)nblk * npts))) { set_error("dqc_int1e_potential: out of memory"); return rc; }
    hipLaunchKernelGGL(int1e_potential_kernel, dim3((unsigned)nblk, (unsigned)ny), dim3(POT_BLOCK), 0, st, d_part, ds, d_cao, d_dcart,
                       ncart, d_points, npts);
    DQC_CHECK_LAUNCH();
    hipLaunchKernelGGL(int1e_potential_sum, dim3((unsigned)((npts + 63) / 64)), dim3(64), 0, st, d_out, (const double *)d_part, (int)nblk,
                       npts);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

int dqc_df_grad(double *d_grad, const double *d_dcart, const double *d_ccart, const int *atm, int natm, const int *bas,
                int nbas, const double *env, int nenv, int sh0, int sh1, int k0, int k1, void *stream) {
    // gradient of the density-fitted Coulomb energy E_J = 1/2 t^T M^-1 t (t_k = sum D_ij (ij|k), M = (k|l), c = M^-1 t):
    //   d_grad (natm, 3) += sum D_ij c_k d(ij|k) - 1/2 sum c_k c_l d(k|l)
    // over the CONCATENATED tables (orbital shells [sh0, sh1), auxiliary shells [k0, k1)); d_dcart (ncart, ncart) and
    // d_ccart (ncart): density matrix and fit coefficients in the Cartesian basis of ALL shells of the table
    // (zero outside the orbital block / auxiliary segment).
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    GradJob j;
    j.who = "dqc_df_grad";
    Basis &b = j.b;
    int rc = parse_basis(b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    if (sh0 < 0 || sh1 > nbas || sh0 > sh1 || k0 < 0 || k1 > nbas || k0 > k1) { set_error("dqc_df_grad: shell ranges outside the table"); return DQC_EINVAL; }
    if (sh0 == sh1 || k0 == k1) return DQC_OK;
    const int N = nbas;
    cart_offsets(b, N, j.cao, j.ncart);
    j.cao.resize(3 * N + 1, 0);
    j.rows.assign(3 * N + 1, 0);
    for (int i = 0; i < N; i++) j.rows[i] = b.shells[i].atom;
    append_centre_companions(b, N);
    // GRAD mode contracts CARTESIAN blocks: the unit function is the Cartesian s function 1 (df.hip uses sqrt(4 pi) because there
    // the l = 0 solid-harmonic factor is applied)
    const int unit = append_unit_shell(b, 1.0);
    HostPairs h3up, h3down, h2up, h2down;
    build_pairs_ordered(b, h3up, N + sh0, N + sh1, sh0, sh1);
    build_pairs_ordered(b, h3down, 2 * N + sh0, 2 * N + sh1, sh0, sh1);
    build_pairs_ordered(b, h2up, N + k0, N + k1, unit, unit + 1);
    build_pairs_ordered(b, h2down, 2 * N + k0, 2 * N + k1, unit, unit + 1);
    build_pairs(b, j.hket, k0, k1, unit);
    j.passes = {{&h3up, +1, 1, launch_grad_df3c<>}, {&h3down, -1, 1, launch_grad_df3c<>},
                {&h2up, +1, 2, launch_grad_df2c<>}, {&h2down, -1, 2, launch_grad_df2c<>}};
    j.nrow = natm; j.norig = N; j.og.ccart = d_ccart;
    return run_grad_job(j, d_dcart, d_grad, (size_t)natm * 3, add_rows, st);
}

int dqc_df_grad3(double *d_grad, const double *d_z, size_t z_doubles, const double *d_g, const int *atm, int natm, const int *bas,
                 int nbas, const double *env, int nenv, int sh0, int sh1, int k0, int k1, void *stream) {
    // the expression dqc_df_grad differentiates, with general densities in place of D_ij c_k and c_k c_l:
    //   d_grad (natm, 3) += sum Z[i, j, k] d(ij|k) - 1/2 sum G[k, l] d(k|l)
    // over the CONCATENATED tables (orbital shells [sh0, sh1), auxiliary shells [k0, k1)).  d_z (no, no, nk), symmetric in i, j, the
    // auxiliary index fastest, and d_g (nk, nk), symmetric: over the Cartesian functions of those two shell ranges ALONE (no and nk
    // of them).  A null d_z or d_g skips its term, so that Z can be walked in blocks of auxiliary shells with G passed once.
    // z_doubles: the doubles behind d_z (0 with a null d_z); fewer than no * no * nk is refused before anything is launched.
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    GradJob j;
    j.who = "dqc_df_grad3";
    Basis &b = j.b;
    int rc = parse_basis(b, atm, natm, bas, nbas, env, nenv, nullptr);
    if (rc) return rc;
    if (sh0 < 0 || sh1 > nbas || sh0 > sh1 || k0 < 0 || k1 > nbas || k0 > k1) { set_error("dqc_df_grad3: shell ranges outside the table"); return DQC_EINVAL; }
    if (sh0 == sh1 || k0 == k1) return DQC_OK;
    const int N = nbas;
    cart_offsets(b, N, j.cao, j.ncart);
    // the kernels address Z and G by the Cartesian offsets of the shells relative to the first shell of each range (EriOut::ao0,
    // aux0): the functions of [sh0, sh1) and of [k0, k1) are all they can reach
    const size_t no = (size_t)((sh1 < N ? j.cao[sh1] : j.ncart) - j.cao[sh0]), nk = (size_t)((k1 < N ? j.cao[k1] : j.ncart) - j.cao[k0]);
    if ((d_z != nullptr || z_doubles != 0) && z_doubles < no * no * nk) {
        set_error("dqc_df_grad3: Z is smaller than the (orbital, orbital, auxiliary) Cartesian block of the shell ranges");
        return DQC_EINVAL;
    }
    if (d_z == nullptr && d_g == nullptr) return DQC_OK;
    if (d_grad == nullptr) { set_error("dqc_df_grad3: null output"); return DQC_EINVAL; }
    const int ao0 = j.cao[sh0], aux0 = j.cao[k0];
    j.cao.resize(3 * N + 1, 0);
    j.rows.assign(3 * N + 1, 0);
    for (int i = 0; i < N; i++) j.rows[i] = b.shells[i].atom;
    append_centre_companions(b, N);
    const int unit = append_unit_shell(b, 1.0);  // (the Cartesian s function 1: dqc_df_grad)
    HostPairs h3up, h3down, h2up, h2down;
    if (d_z != nullptr) {
        build_pairs_ordered(b, h3up, N + sh0, N + sh1, sh0, sh1);
        build_pairs_ordered(b, h3down, 2 * N + sh0, 2 * N + sh1, sh0, sh1);
        j.passes.push_back({&h3up, +1, 3, launch_grad_df3c<ERI_OUT_GRAD3>});
        j.passes.push_back({&h3down, -1, 3, launch_grad_df3c<ERI_OUT_GRAD3>});
    }
    if (d_g != nullptr) {
        build_pairs_ordered(b, h2up, N + k0, N + k1, unit, unit + 1);
        build_pairs_ordered(b, h2down, 2 * N + k0, 2 * N + k1, unit, unit + 1);
        j.passes.push_back({&h2up, +1, 4, launch_grad_df2c<ERI_OUT_GRAD3>});
        j.passes.push_back({&h2down, -1, 4, launch_grad_df2c<ERI_OUT_GRAD3>});
    }
    build_pairs(b, j.hket, k0, k1, unit);
    j.nrow = natm; j.norig = N; j.og.ccart = d_g;
    j.og.nao = (int)no; j.og.naux = (int)nk; j.og.ao0 = ao0; j.og.aux0 = aux0;
    return run_grad_job(j, d_z, d_grad, (size_t)natm * 3, add_rows, st);
}

}  // extern "C"
