// grad_launch.hpp -- the class launchers of the GRAD output modes, shared by the translation units that instantiate them: grad.hip
// (ERI_OUT_GRAD, ERI_OUT_GRAD3 and the host driver run_grad_job) and grad2.hip (ERI_OUT_GRAD2, the bilinear form of dqc_eri_grad2 --
// 200 further compile-time classes, kept out of grad.hip so that the two halves compile side by side).
#pragma once
#include "eri_generic.hpp"

namespace dqc {

constexpr int GRAD_LMAX = 3;  // orbital shells up to f in the compile-time classes (companions up to g); above: eri_generic.hpp

struct GradCtx {
    DevShells ds;
    DevPairs dbra, dket;
    const HostPairs *hbra, *hket;
    EriOut og;
    DevPool *pool = nullptr;  // stream-ordered pool for the wave tables (nullptr: flat task maps)
    SideStreams *side = nullptr;  // class launches dealt round-robin to the side streams (common.hpp)
    int wmap_depth = 1 << 30;  // class pairs whose deepest contraction has at least this many primitive quartets take the wave map
};

// MODE: ERI_OUT_GRAD, ERI_OUT_GRAD3 for the passes of dqc_df_grad3 (gmode 3 and 4), or ERI_OUT_GRAD2 for those of dqc_eri_grad2
template <int LA, int LB, int LC, int LD, int MODE = ERI_OUT_GRAD>
static int launch_grad_class(const GradCtx &c, hipStream_t st) {
    using Cfg = EriCfg<LA, LB, LC, LD>;
    const int cb = LA * 8 + LB, ck = LC * (LC + 1) / 2 + LD;
    const int nb = c.hbra->cls_count[cb], nk = c.hket->cls_count[ck];
    if (nb == 0 || nk == 0 || hl_forced()) return 0;
    const long long ntask = (long long)nb * nk;
    const long long nblk = eri_num_blocks<Cfg>(nb, nk, ntask);
    auto kern = eri_kernel<LA, LB, LC, LD, MODE>;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS_BYTES_G);
    if (c.side != nullptr) st = c.side->take();
    // (only where the class pair's deepest contraction -- first pair of each class: the lists are sorted by depth -- is worth splitting)
    const int dmax = (c.hbra->pp_off[c.hbra->cls_start[cb] + 1] - c.hbra->pp_off[c.hbra->cls_start[cb]]) *
                     (c.hket->pp_off[c.hket->cls_start[ck] + 1] - c.hket->pp_off[c.hket->cls_start[ck]]);
    if (Cfg::TPQ <= 16 && c.pool != nullptr && dmax >= c.wmap_depth) {
        // depth-binned wave map (eri_core.hpp: eri_split_lanes, eri_wave_table): the deep (companion, s) x (s, s) contractions were
        // serial chains in single lane groups
        std::vector<WaveRun> runs;
        EriOut o2 = c.og;
        const long long nwave = eri_wave_runs(runs, o2.wbin, *c.hbra, c.hbra->cls_start[cb], nb, *c.hket, c.hket->cls_start[ck], nk, Cfg::TPQ);
        if (nwave == 0) return 0;
        WaveRun *d_runs = nullptr;
        if (c.pool->upload(&d_runs, runs, st)) { set_error("dqc_eri_grad: device upload failed"); return DQC_ENOMEM; }
        o2.wruns = d_runs;
        o2.nruns = (int)runs.size();
        hipLaunchKernelGGL(kern, dim3((unsigned)((nwave + 3) / 4)), dim3(256), Cfg::LDS_BYTES_G, st, (double *)nullptr, c.ds, c.dbra, c.dket,
                           c.hbra->cls_start[cb], nb, c.hket->cls_start[ck], nk, 0, nwave, o2);
        DQC_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), Cfg::LDS_BYTES_G, st, (double *)nullptr, c.ds, c.dbra, c.dket,
                       c.hbra->cls_start[cb], nb, c.hket->cls_start[ck], nk, 0, ntask, c.og);
    DQC_CHECK_LAUNCH();
    return 0;
}

template <int LA, int LB, int MODE = ERI_OUT_GRAD>
static int launch_grad_bra(const GradCtx &c, hipStream_t st) {
    int rc;
#define DQC_GK(LC, LD) \
    if ((rc = launch_grad_class<LA, LB, LC, LD, MODE>(c, st))) return rc;
    DQC_GK(0, 0) DQC_GK(1, 0) DQC_GK(1, 1) DQC_GK(2, 0) DQC_GK(2, 1) DQC_GK(2, 2) DQC_GK(3, 0) DQC_GK(3, 1) DQC_GK(3, 2) DQC_GK(3, 3)
#undef DQC_GK
    return 0;
}

// the classes outside the compile-time set (h companions, g shells) through the runtime kernel; ket pairs (lc >= ld), or
// (auxiliary shell, unit) when `df`
template <int MODE = ERI_OUT_GRAD>
static int launch_grad_generic(const GradCtx &c, bool df, int lbmax, hipStream_t st) {
    for (int la = 0; la <= DQC_LMAX + 1; la++)
        for (int lb = 0; lb <= lbmax; lb++)
            for (int lc = 0; lc <= DQC_LMAX; lc++)
                for (int ld = 0; ld <= (df ? 0 : lc); ld++) {
                    if (!hl_forced() && la <= GRAD_LMAX + 1 && lb <= GRAD_LMAX && lc <= GRAD_LMAX) continue;
                    const int cb = la * 8 + lb, ck = lc * (lc + 1) / 2 + ld;
                    int rc = launch_hl<MODE>(nullptr, c.ds, c.dbra, c.dket, c.hbra->cls_start[cb], c.hbra->cls_count[cb],
                                                     c.hket->cls_start[ck], c.hket->cls_count[ck], 0, c.og, la, lb, lc, ld, st);
                    if (rc) return rc;
                }
    return 0;
}

// every four-index class of one pass: the runtime kernel's, then the compile-time ones
template <int MODE = ERI_OUT_GRAD>
static int launch_grad_all(const GradCtx &c, hipStream_t st) {
    int rc;
    if ((rc = launch_grad_generic<MODE>(c, false, DQC_LMAX, st))) return rc;
#define DQC_GB(LA) \
    if ((rc = launch_grad_bra<LA, 0, MODE>(c, st)) || (rc = launch_grad_bra<LA, 1, MODE>(c, st)) || (rc = launch_grad_bra<LA, 2, MODE>(c, st)) || (rc = launch_grad_bra<LA, 3, MODE>(c, st))) return rc;
    DQC_GB(0) DQC_GB(1) DQC_GB(2) DQC_GB(3) DQC_GB(4)
#undef DQC_GB
    return 0;
}

// grad2.hip: launch_grad_all<ERI_OUT_GRAD2>
int launch_grad2_all(const GradCtx &c, hipStream_t st);

}  // namespace dqc
