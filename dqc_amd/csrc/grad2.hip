// grad2.hip -- the ERI_OUT_GRAD2 instantiations of the Rys quartet kernels: the nuclear-gradient contraction of grad.hip as the
// symmetric bilinear form of TWO Cartesian matrices (eri_core.hpp), for the two-particle densities that are products of different
// matrices -- the SCF density with a relaxed difference density, the symmetric and antisymmetric transition densities of an excited
// state with themselves (dqc_amd/excited.py).  The four-index classes alone: the compile-time ones s ... f (companions up to g) and
// the runtime kernel for g shells and h companions.  The host side (dqc_eri_grad2: gates, companions, pair lists, the GradJob and
// run_grad_job) is in grad.hip; this translation unit exists so that its 200 classes compile beside those of grad.hip.
#include "grad_launch.hpp"

namespace dqc {

int launch_grad2_all(const GradCtx &c, hipStream_t st) {
    // the Boys table of the closed-form classes is one device copy per translation unit (eri_core.hpp): run_grad_job has uploaded the
    // one of grad.hip, the kernels instantiated here read this one
    int rc = boys_table_ensure();
    if (rc) return rc;
    return launch_grad_all<ERI_OUT_GRAD2>(c, st);
}

}  // namespace dqc
