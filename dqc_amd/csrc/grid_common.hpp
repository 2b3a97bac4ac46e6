// grid_common.hpp -- what the density and the Vxc translation units share (the f64 MFMA wrapper and fragment layout of mfma_tile.hpp,
// the functionals, streaming loads).
#pragma once
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "mfma_tile.hpp"
#include "xc_funcs.hpp"

namespace dqc {

// Loads of data that a launch reads exactly ONCE (the rows of the AO arrays in the factor-form density pass, 2.3 GB per launch for
// the 20-atom molecule): non-temporal, so that the stream does not allocate in L2 and the Infinity Cache on its way through.  The
// value loaded is the same; anything read more than once (L, L^T, the mailboxes) keeps the default policy.  Measured per kernel
// (docs/LOG_r18.md): density_roles_kernel<3, 13> 394.8 -> 354.9 us; the same policy on the Vxc producers' buffer loads (aux = 2)
// changed nothing (507.8 -> 508.6 us): they keep plain loads.  j_stream_kernel's tile loads lost 9 % to it (323.3 -> 352.5 us) while an
// instruction covered half lines, and take it since they cover whole ones (csrc/jk.hip, docs/LOG_r28.md).
typedef double v2d __attribute__((ext_vector_type(2)));
DQC_DEV double2 load_once16(const double *p) {  // p 16-byte aligned
    const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(p));
    return make_double2(v.x, v.y);
}
DQC_DEV double load_once8(const double *p) { return __builtin_nontemporal_load(p); }

}  // namespace dqc
