// mgvcycle.hip - C ABI (include/mgvcycle.h) and level schedule of the MI355X multigrid cycle.
//
// Reference behaviour reproduced (JuliaInv/Multigrid.jl v0.8.0):
//   recursiveCycle  src/Multigrid/MGcycle.jl:1-118   (operation order: SURVEY.md 3.2)
//   relax           src/Multigrid/MGcycle.jl:122-136
//   solveCoarsest   src/Multigrid/MGcycle.jl:138-181 (default branch, l.177)
//   solveMG         src/Multigrid/SolveFuncs.jl:3-39
// The hierarchy is resident in HBM; the host only sequences kernel launches on one HIP stream.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // declarations only: librccl is dlopen'ed by mg_dist_* (single-GPU users do not depend on it)

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/mgvcycle.h"
#include "mg_kernels.hpp"
#include "mg_march27.hpp"
#include "mg_marchr.hpp"
#include "mg_small.hpp"
#include "mg_complex.hpp"
#include "mg_krvec.hpp"
#include "mg_cxvec.hpp"
#include "mg_cxblk_coarse.hpp"
#include "mg_dd.hpp"
#include "mg_vanka.hpp"
#include "mg_dense_inv.hpp"
#include "mg_krylov_host.hpp"   // host only: KrylovReport, HessenbergLsq, RelaxLsq / pinv_sym, SmallMat / sm_*


// One translation unit in parts (the 6 800-line file split by responsibility; the order is the dependency order):
#include "mg_types.inc"      // Options, DevBuf, Csr, Level, mg_hierarchy
#include "mg_launch.inc"     // byte accounting, profiling slots, kernel launchers
#include "mg_transport.inc"  // RCCL loader, host-staged plug-in: the collectives of both sharded forms
#include "mg_ghost.inc"      // ghost-layer form of the sharded cycle: exchange, validity bookkeeping, global norms
#include "mg_vanka.inc"      // the Vanka cell-block smoother: per-level core of relaxation type 2, extern "C" mg_vanka_*
#include "mg_schedule.inc"   // FGMRES relaxation, cycle_level, HIP graphs, solve loop
#include "mg_krylov.inc"     // PCG / BiCGSTAB / FGMRES and block variants
#include "mg_formats.inc"    // upload, format builders, scratch
#include "mg_dense_inv.inc"  // the dense inverse with partial pivoting on the device: work set, chain of launches
#include "mg_complex.inc"    // ComplexF64 hierarchies: generic-CSR kernels' launchers, cycle, solve, and their extern "C" entry points
#include "mg_complex_krylov.inc"   // extern "C": ComplexF64 BiCGSTAB / FGMRES on a system operator of their own, their fused vector passes
#include "mg_cabi.inc"       // extern "C": the single-GPU API and its ghost-layer form (mg_ghost_*)
#include "mg_dist.inc"       // extern "C": the native multi-GPU sequencer (halo form)
#include "mg_dist_krylov.inc"   // extern "C": PCG / BiCGSTAB / FGMRES on the sharded halo form, their fused vector passes
#include "mg_dd.inc"         // extern "C": the multiplicative Schwarz preconditioner of src/DomainDecomposition (mg_dd_*)
