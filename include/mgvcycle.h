/*
 * mgvcycle.h - C ABI of libmgvcycle.so, the MI355X (gfx950) multigrid-cycle library.
 *
 * Drop-in boundary for the hot path of JuliaInv/Multigrid.jl (reference @ v0.8.0):
 *   recursiveCycle  src/Multigrid/MGcycle.jl:1-118      -> mg_cycle_*
 *   relax           src/Multigrid/MGcycle.jl:122-136    -> fused inside mg_cycle_*
 *   solveCoarsest   src/Multigrid/MGcycle.jl:138-181    -> fused inside mg_cycle_* (default branch l.177)
 *   solveMG         src/Multigrid/SolveFuncs.jl:3-39    -> mg_solve_*
 *   SpMatMul        src/Multigrid/SpMatMul.jl:4-26      -> mg_spmv_*
 *   addVectors      src/Multigrid/SpMatMul.jl:29-37     -> fused into the SpMV epilogues
 *   MGparam         src/Multigrid/MGdef.jl:91-116       -> mg_hierarchy (opaque) + mg_set_*
 *   adjustMemoryForNumRHS  src/Multigrid/MGsetup.jl:166-223 -> mg_set_nrhs
 *   replaceMatrixInHierarchy (numeric part) MGsetup.jl:226-270 -> mg_replace_values_FP64
 *   clear!/destroyCoarsestLU  MGdef.jl:179-206          -> mg_destroy
 *
 * Calling convention follows the reference's own ccall idiom (src/Multigrid/parRelax.jl:61-64,
 * deps/src/parRelax.h:7-43): sparse operators are passed exactly as Julia's SparseMatrixCSC holds
 * them - colptr/rowval as 1-based Int64, nzval as Float64 - and the library subtracts 1; scalars are
 * long long / double; symbols carry the _FP64_INT64 suffix.  Unlike the reference's void functions,
 * every entry point returns an int status (MG_OK == 0) and mg_last_error() returns the message.
 *
 * The reference stores every operator TRANSPOSED (MGdef.jl:75-77), so the CSC arrays of AT are the
 * CSR arrays of A: colptr = row pointers, rowval = column indices.  "n_rows" below is therefore
 * length(colptr)-1 = size(AT,2) and "n_cols" is size(AT,1).
 *
 * Ownership: the caller owns every host array; the library copies the hierarchy to HBM inside
 * mg_set_* / mg_finalize and retains no host pointer.  b is read-only, x is in/out in the caller's
 * buffer (the in-place contract test/Multigrid/testGMG.jl:54-55 asserts).  A handle is not
 * thread-safe (neither is MGparam: the F-cycle mutates it, MGcycle.jl:82-84).
 */
#ifndef MGVCYCLE_H
#define MGVCYCLE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_hierarchy mg_hierarchy;

/* status codes */
#define MG_OK 0
#define MG_ERR_INVALID 1   /* bad argument / inconsistent hierarchy */
#define MG_ERR_HIP 2       /* HIP runtime error (no device, out of memory, launch failure) */
#define MG_ERR_STATE 3     /* call out of order (e.g. cycle before finalize) */
#define MG_ERR_UNSUPPORTED 4

/* operator selector for mg_set_operator / mg_spmv / mg_replace_values */
#define MG_OP_A 0 /* As[level]  : n_l x n_l                                  */
#define MG_OP_P 1 /* Ps[level]  : CSR of P, n_l rows  x n_{l+1} cols         */
#define MG_OP_R 2 /* Rs[level]  : CSR of R, n_{l+1} rows x n_l cols          */

/* kernel selector for mg_time_op_dev_FP64 / mg_profile_get */
#define MG_K_SPMV 0     /* y = alpha*A*x + beta*y          (SpMatMul.jl:4-13)          */
#define MG_K_RESIDUAL 1 /* r = b - A*x                     (MGcycle.jl:58-60 fused)    */
#define MG_K_SMOOTH 2   /* x' = x + d.*(b - A*x)           (MGcycle.jl:128-131 fused)  */
#define MG_K_RESTRICT 3 /* bc = R*r                        (MGcycle.jl:66)             */
#define MG_K_PROLONG 4  /* x += P*xc                       (MGcycle.jl:90)             */
#define MG_K_DSCALE 5   /* x = d.*b (first sweep from x=0) (MGcycle.jl:134)            */
#define MG_K_COARSE 6   /* xc = LU \ bc                    (MGcycle.jl:177)            */
#define MG_K_NORM 7     /* ||r||^2                         (SolveFuncs.jl:30)          */
#define MG_K_SMOOTH_PROLONG 8 /* small levels (round 6): x + P*xc formed in LDS inside the first post-smoothing sweep's launch (grid27_small_prolong_smooth; MGcycle.jl:90-102); profile slot only.  (The fine-level form of rounds 2-5 - the prolongation inside the marching sweep's staging - was slower in every round and is retired.)  A small level's residual + restriction as one launch (grid27_small_resid_restrict) is counted under MG_K_RESTRICT */
#define MG_K_SMOOTH_RESIDUAL 9 /* t = x + d.*(b - A*x) and r = b - A*t in one pass (MGcycle.jl:129-131 + 58-60 / SolveFuncs.jl:26-27) */
#define MG_K_SMOOTH_RESIDUAL_NORM 10 /* the same pass in the solve loop: last post-smoothing sweep + the stopping test's residual: ||r||^2 and t + d.*r out (SolveFuncs.jl:26-30); profile slot only */
#define MG_K_FOUR_STAGE 11 /* solve loop, fine level: the last post-smoothing sweep + stopping-test residual of step k AND the second pre-smoothing sweep + residual of step k+1 in one pass (SolveFuncs.jl:24-37 around MGcycle.jl:26-31,54-60): x, b in; t', r' and ||r||^2 out; profile slot only */
#define MG_K_GHOST 12 /* ghost-layer form of the sharded cycle: pack + (host-staged / dry transport) unpack kernels of one exchange on the compute stream; profile slot only */
#define MG_K_COUNT 13

/* ---- lifecycle ---------------------------------------------------------------------------- */

/* Allocate an empty hierarchy of `nlevels` levels (length(param.As)) on HIP device `device_id`,
 * sized for `nrhs` right-hand sides.  Levels are 1-based in every call below, as in the reference. */
int mg_create(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out);

/* Upload one operator from Julia's CSC-of-the-transpose arrays (1-based Int64). */
int mg_set_operator_FP64_INT64(mg_hierarchy* h, long long level, long long which,
                               long long n_rows, long long n_cols,
                               const long long* colptr, const long long* rowval, const double* nzval);

/* relaxPrecs[level] (length n_level) and relaxPre(level)/relaxPost(level) evaluated by the host
 * (they are Julia functions of the level, MGdef.jl:98-99). */
int mg_set_relax_FP64(mg_hierarchy* h, long long level, const double* d, long long n,
                      long long relaxPre, long long relaxPost);

/* Launch-bound coarse sub-cycles (from the first level of at most `graph_max_rows` rows*nrhs down, option
 * "graph_max_rows", default 300000; "no_graph" switches it off) are captured once into HIP graphs and replayed: the
 * reference has no counterpart (its recursion is host code, MGcycle.jl:1-118).  Counters for tests and tuning:
 * *launches = graph replays so far, *graphs = graphs currently cached.  Graphs are dropped by every call that
 * changes the hierarchy. */
int mg_graph_launches(mg_hierarchy* h, long long* launches, long long* graphs);

/* Optional performance hint (results are unchanged): the rows of As[level] are the nodes of an x-fastest
 * n1 x n2 x n3 regular grid (param.Meshes[level].n .+ 1 for geometric multigrid, MGsetup.jl:54).  Lets the
 * library walk the row blocks in L2-sized y-tiles when three grid planes of the gathered vector do not fit
 * an XCD's L2 (block right-hand sides, grids beyond ~400^2 nodes per plane).  n3 = 1 for 2-D. */
int mg_set_grid_hint(mg_hierarchy* h, long long level, long long n1, long long n2, long long n3);

/* Override one format-selection switch of THIS handle (DESIGN.md section 3 lists them; key = the environment name
 * without the MG_ prefix, lower case: "no_rowclass", "no_tile", "tile_min_wg", "nt", ...).  The environment itself is
 * read once, inside mg_create; nothing on the launch path reads it.  Applies to operators uploaded after the call
 * (call it right after mg_create), e.g. mg_set_option(h, "no_rowclass", 1) forces the streaming CSR formats. */
int mg_set_option(mg_hierarchy* h, const char* key, double value);

/* relaxType: 0 = pointwise relaxPrecs ("Jac", "SPAI": relax(), MGcycle.jl:122-136);
 * 1 = "Jac-GMRES": FGMRES_relaxation with npre/npost inner directions, preconditioned by relaxPrecs
 * (FGMRES.jl:48-126, MGcycle.jl:35-38,48-50,96-98);
 * 2 = the Vanka cell-block smoother (RelaxVankaFacesColor, MGcycle.jl:51-52,99-100) with the blocks mg_set_vanka_FP64 bound to
 * every non-coarsest level: npre / npost in-place iterations (a count of 0: no sweep), no fused passes and no graph replay.
 * FP64 handles, one right-hand side, V / W / F cycles (MG_ERR_UNSUPPORTED otherwise).  Call before mg_finalize. */
int mg_set_relax_type(mg_hierarchy* h, long long relaxType);

/* Bind the Vanka blocks of `level` (relaxation type 2): n[dim] cells of the level's RegularMesh, VankaType 1 (FULL_VANKA_RB),
 * 3 (ECON_VANKA_RB) or 5 (FULL_VANKA_ADD), D_blocks as for mg_vanka_create_FP64_INT64.  The level's operator must have been
 * uploaded (mg_set_operator_FP64_INT64) and have sum(nf) [+ prod(n)] rows; the sweep counts are those of mg_set_relax_FP64.
 * mg_finalize fails with MG_ERR_STATE if type 2 is set and a non-coarsest level has no blocks. */
int mg_set_vanka_FP64(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure,
                      long long VankaType, const float* D_blocks);

/* cycleType: 'V', 'W', 'F' (MGcycle.jl:78-85) or 'K' (2-step FGMRES recursion, MGcycle.jl:72-76). */
int mg_set_cycle_type(mg_hierarchy* h, long long cycleType);

/* Coarsest solve, default branch `z = param.LU\b` (MGcycle.jl:177): the host factors the coarsest
 * operator (UMFPACK in the reference, MGsetup.jl:350) and hands over the explicit inverse,
 * column-major n x n, applied on device as a dense product. */
int mg_set_coarse_dense_inverse_FP64(mg_hierarchy* h, long long n, const double* Ainv_colmajor);

/* The same solve from SPARSE factors, for coarsest levels too large for an explicit inverse: the layout of the
 * reference's native applier (deps/src/parLU.cpp:120-190 / setupLUFactor, parallelJuliaSolver.jl:113-148): CSR L
 * with the diagonal LAST in every row, CSR U with the diagonal FIRST, 1-based Int64 pointers/indices, p and q with
 * A[p,q] = L*U, so that x[q] = U \ (L \ b[p]).  Applied by one workgroup walking the dependency levels. */
int mg_set_coarse_lu_FP64_INT64(mg_hierarchy* h, long long n, const long long* Lptr, const long long* Lcol,
                                const double* Lval, const long long* Uptr, const long long* Ucol,
                                const double* Uval, const long long* p, const long long* q);

/* coarseSolveType "GMRES" (MGcycle.jl:152-168): the coarsest level is solved by one restart of Jacobi-preconditioned
 * FGMRES(10) with tol 0.01 from x = 0; d = relaxParam ./ diag(A_c) is what defineCoarsestAinv keeps in param.LU
 * (MGsetup.jl:334).  A block of right-hand sides takes the reference's blockFGMRES branch (MGcycle.jl:164-166): block
 * flexible GMRES(10), one restart, Frobenius residual estimate <= 1e-2, same preconditioner per column. */
int mg_set_coarse_gmres_FP64(mg_hierarchy* h, long long n, const double* d);

/* Validate the hierarchy (shapes chain, every level complete), build the row-block partitions,
 * allocate the per-level b/r/x scratch (CYCLEmem, MGdef.jl:56-60). */
int mg_finalize(mg_hierarchy* h);

/* adjustMemoryForNumRHS: re-size the scratch when the number of RHS columns changes. */
int mg_set_nrhs(mg_hierarchy* h, long long nrhs);

/* Replace the numerical values of an operator whose sparsity is unchanged (nnz must match). */
int mg_replace_values_FP64(mg_hierarchy* h, long long level, long long which,
                           const double* nzval, long long nnz);

/* replaceMatrixInHierarchy on the device (MGsetup.jl:226-270): new fine values on the unchanged sparsity, then
 * per level relaxPrecs[l] (relaxKind 0: Jac omega/diag, 1: SPAI omega*diag/colnorm^2; omega[l] per level) and the
 * Galerkin product As[l+1] = Ps[l]*As[l]*Rs[l] on the fixed patterns (rows of As[l+1] of any length: 2048 target columns
 * at a time; deterministic - the same sums in the same order on every run).  The coarsest factorisation stays on the host: fetch the
 * coarsest values (mg_get_values_FP64), factor, mg_set_coarse_dense_inverse_FP64, mg_finalize - unless the option
 * "coarse_device_inverse" is set and a dense inverse installed: then it is rebuilt here, in HBM (mg_build_coarse_dense_inverse_FP64).
 * A coarse operator As[l+1] with a row whose stored columns descend anywhere is refused (MG_ERR_UNSUPPORTED, found at upload,
 * before anything is written): the kernel finds its target columns by binary search in that row. */
int mg_rap_FP64(mg_hierarchy* h, const double* fine_nzval, long long nnz, long long relaxKind,
                const double* omega, long long* levels_done);
int mg_get_values_FP64(mg_hierarchy* h, long long level, long long which, double* out, long long nnz);
int mg_get_relax_FP64(mg_hierarchy* h, long long level, double* out, long long n);

int mg_destroy(mg_hierarchy* h);

/* ---- the hot path, host buffers (what the Julia glue ccalls) -------------------------------- */

/* One cycle x <- recursiveCycle(param,b,x,1).  b, x: column-major n x nrhs (Julia Array{Float64}).
 * x_is_zero: 1 = caller guarantees x==0 (preconditioner closure, SolveFuncs.jl:59), 0 = x!=0,
 * -1 = decide like the reference does with norm(x)>0 (MGcycle.jl:29). */
int mg_cycle_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                  long long x_is_zero);

/* solveMG: cycles until ||b-Ax||_F/||r0||_F < tol or maxIter (SolveFuncs.jl:14-37).
 * resvec (length maxIter+1, may be NULL) receives r0 and the residual norm after every cycle. */
int mg_solve_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                  double tol, long long maxIter, long long* iters, double* resvec);

/* solveCG_MG (SolveFuncs.jl:104-116): KrylovMethods.cg (v0.6.0, external) preconditioned with one cycle
 * from x = 0 (getMultigridPreconditioner, SolveFuncs.jl:59), vectors resident on device across iterations.
 * nrhs = 1 (a block of right-hand sides: mg_block_pcg_FP64 / mg_block_pcg_dev_FP64 below).  resvec (length maxIter) receives ||r||/||b|| per iteration;
 * flag: 0 converged, -1 maxIter reached, -2 breakdown (alpha = Inf or < 0), -9 b = 0. */
int mg_pcg_FP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol,
                long long maxIter, long long* iters, long long* flag, double* resvec);
int mg_pcg_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, double tol,
                    long long maxIter, long long* iters, long long* flag, double* resvec);

/* solveBiCGSTAB_MG (SolveFuncs.jl:87-101): KrylovMethods.bicgstb (external) with M1 = one cycle from x = 0,
 * M2 = identity.  resvec (length 2*maxIter+1) receives ||r0||/||b|| and two entries per iteration; *nres their
 * number.  flag: 0 converged, -1 maxIter, -2 breakdown, -3 converged on the half step, -9 b = 0.  nrhs = 1 (blocks: mg_block_bicgstab_*). */
int mg_bicgstab_FP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol,
                     long long maxIter, long long* iters, long long* flag, double* resvec,
                     long long* nres);
int mg_bicgstab_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, double tol,
                         long long maxIter, long long* iters, long long* flag, double* resvec,
                         long long* nres);

/* solveGMRES_MG (SolveFuncs.jl:119-133): KrylovMethods.fgmres (external), flexible restarted GMRES(inner) with one
 * cycle from x = 0 as preconditioner.  maxIter counts restarts; resvec (length inner*maxIter) receives the residual
 * estimate after every inner step, *nres their number, *iters the total number of inner steps.  nrhs = 1 (blocks: mg_block_fgmres_*). */
int mg_fgmres_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long inner, double tol,
                   long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
/* the same with b and x in HBM (device pointers), like mg_pcg_dev_FP64 / mg_bicgstab_dev_FP64 */
int mg_fgmres_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long inner, double tol,
                       long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);

/* The block branches of the same three drivers (size(b,2) > 1: KrylovMethods.blockCG / blockBiCGSTB / blockFGMRES,
 * SolveFuncs.jl:95,113,130), nrhs <= 16, every n x nrhs block resident in HBM across iterations.  The package is not
 * vendored: the published algorithms are restated in oracle/mg_oracle.py (O'Leary's block CG with a pseudo-inverse of
 * P'AP; El Guennouni-Jbilou-Sadok block BiCGSTAB, M1 = the cycle; block flexible GMRES with block modified Gram-Schmidt,
 * blocks orthonormalised by Cholesky QR applied twice).  Stopping: max over columns of ||r_j||/||b_j|| <= tol (CG,
 * BiCGSTAB; resmat is maxIter x nrhs row-major, resvec as for the single-vector driver), Frobenius norm for FGMRES.
 * Flags as for the single-vector drivers.  b / x: column-major host blocks, or row-major [n][nrhs] device blocks (_dev). */
int mg_block_pcg_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                      long long maxIter, long long* iters, long long* flag, double* resmat);
int mg_block_pcg_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs, double tol,
                          long long maxIter, long long* iters, long long* flag, double* resmat);
int mg_block_bicgstab_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                           long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
int mg_block_bicgstab_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs,
                               double tol, long long maxIter, long long* iters, long long* flag, double* resvec,
                               long long* nres);
int mg_block_fgmres_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long inner,
                         double tol, long long maxIter, long long* iters, long long* flag, double* resvec,
                         long long* nres);
int mg_block_fgmres_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs,
                             long long inner, double tol, long long maxIter, long long* iters, long long* flag,
                             double* resvec, long long* nres);

/* ---- the real drivers' passes on their own (tests, callers with loops of their own) ------------------------------------------
 * Each entry runs ONE vector or block pass of the drivers above through the helper the driver itself calls: the same kernel, grid,
 * partial buffers and stream.  h: a finalized real FP64 handle whose drivers are not sharded (MG_ERR_STATE otherwise); n: the length
 * of the caller's vectors, n >= 1 - it need not be the hierarchy's.  Null pointers, n < 1, k outside 1..16, i outside 0..63:
 * MG_ERR_INVALID.  A refusal launches nothing and leaves the handle usable.  Vectors and blocks (row-major [n][k]) are device
 * pointers; *_host arguments are host pointers, and an entry that fills one has drained the handle's stream when it returns.  The
 * others enqueue on the handle's stream and return.
 *   dot       *out_host = x'y                                norm      *out_host = ||x||_2
 *   axpby     y = a x + b y ; y is not read when b == 0      cg_p      p = z + beta p
 *   cg_update x += alpha p ; r -= alpha Ap ; with rnorm_host != NULL also *rnorm_host = ||r|| of the new r, from the same pass
 *   mgs_step  w -= (*hk_dev) v ; *out_dev = w'u of the new w (u == NULL: w'w)
 *   mgs_chain V: i + 2 vectors n apart, w = the last: h_k = w'V_k, w -= h_k V_k for k = 0..i in turn, then w /= ||w|| unless
 *             ||w|| == 0; h_host receives h_0 .. h_i and ||w||^2 (i + 2 doubles) - the orthogonalisation of one FGMRES inner step
 *   blk_gram  G_host (k x k row-major) = X'Y                 blk_comb  out = s add + in C_host (k x k row-major); add may be
 *             NULL (then s is ignored); out may be in or add */
int mg_kry_dot_dev_FP64(mg_hierarchy* h, const double* x_dev, const double* y_dev, long long n, double* out_host);
int mg_kry_norm_dev_FP64(mg_hierarchy* h, const double* x_dev, long long n, double* out_host);
int mg_kry_axpby_dev_FP64(mg_hierarchy* h, double a, const double* x_dev, double b, double* y_dev, long long n);
int mg_kry_cg_update_dev_FP64(mg_hierarchy* h, double alpha, const double* p_dev, const double* Ap_dev, double* x_dev,
                              double* r_dev, long long n, double* rnorm_host);
int mg_kry_cg_p_dev_FP64(mg_hierarchy* h, double beta, const double* z_dev, double* p_dev, long long n);
int mg_kry_mgs_step_dev_FP64(mg_hierarchy* h, const double* hk_dev, const double* v_dev, double* w_dev, const double* u_dev,
                             long long n, double* out_dev);
int mg_kry_mgs_chain_dev_FP64(mg_hierarchy* h, double* V_dev, long long n, long long i, double* h_host);
int mg_kry_blk_gram_dev_FP64(mg_hierarchy* h, const double* X_dev, const double* Y_dev, long long n, long long k,
                             double* G_host);
int mg_kry_blk_comb_dev_FP64(mg_hierarchy* h, double* out_dev, const double* add_dev, double s, const double* in_dev,
                             const double* C_host, long long n, long long k);

/* Mixed-precision preconditioner hook of getMultigridPreconditioner (SolveFuncs.jl:52-58): a Float32 block against the
 * Float64 hierarchy - bl .= b; z .= 0; recursiveCycle(param,bl,z,1); z2 .= z.  Column-major n x nrhs host blocks. */
int mg_cycle_mixed_FP32(mg_hierarchy* h, const float* b32, float* z32, long long n, long long nrhs);

/* Page-lock / release a long-lived host array (the preconditioner's z = param.memCycle[1].x, a solver's b and x) so the
 * host-pointer entry points above copy it at full PCIe rate.  The caller owns the lifetime: unregister before the
 * array is freed or resized (hipHostRegister / hipHostUnregister). */
int mg_host_register(void* ptr, long long bytes);
int mg_host_unregister(void* ptr);

/* target = beta*target + alpha*Op*x on one level (SpMatMul.jl:4-13); column-major host blocks. */
int mg_spmv_FP64(mg_hierarchy* h, long long level, long long which, double alpha, const double* x,
                 double beta, double* y, long long nrhs);

/* ---- the hot path, device-resident buffers -------------------------------------------------- */
/* Same semantics with b/x already in HBM (hipMalloc'd or torch tensors' data_ptr).  Blocks with
 * nrhs>1 use the library's device layout: row-major [n][nrhs].  Work is enqueued on the library's
 * stream; the call returns after the stream has drained (synchronous from the host's view).
 * The library's stream is non-blocking: it does NOT order against the caller's streams.  Whatever the caller still has in
 * flight for these buffers (a fill, a copy, the kernel that produced b) must be complete on entry - synchronise the
 * producing stream first (the Python binding does: device.py::_sync_torch), or hand the library that stream (mg_set_stream). */
int mg_cycle_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n,
                      long long nrhs, long long x_is_zero);
int mg_solve_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n,
                      long long nrhs, double tol, long long maxIter, long long* iters,
                      double* resvec);
int mg_spmv_dev_FP64(mg_hierarchy* h, long long level, long long which, double alpha,
                     const double* x_dev, double beta, double* y_dev, long long nrhs);
/* Fused forms used inside the cycle, exposed for kernel-level parity tests:
 *   MG_K_RESIDUAL: out = b - A*x ;  MG_K_SMOOTH: out = x + d.*(b - A*x)   (out must not alias x). */
int mg_fused_dev_FP64(mg_hierarchy* h, long long level, long long kernel, const double* b_dev,
                      const double* x_dev, double* out_dev, long long nrhs);
/* Two stages in one pass over level `level` (1-based, not the coarsest): t = x + d.*(b - A*x)  (relax's sweep,
 * MGcycle.jl:129-131) and r = b - A*t (MGcycle.jl:58-60 / SolveFuncs.jl:26-27); optionally xn = t + d.*r (the next
 * cycle's first update) and *norm_r = ||r|| (SolveFuncs.jl:30).  r_dev, xn_dev, norm_r may be NULL.  x, t, r, xn must be
 * four different 16-byte aligned device buffers.  MG_ERR_UNSUPPORTED when the level is not served by the two-stage
 * marching kernel (the cycle then runs the two launches). */
int mg_sweep_residual_dev_FP64(mg_hierarchy* h, long long level, const double* b_dev, const double* x_dev,
                               double* t_dev, double* r_dev, double* xn_dev, double* norm_r);

/* The solve loop's two fine-level passes across the stopping test as ONE four-stage pass (round 4; replaces the pair
 * SolveFuncs.jl:24-37 runs back to back: the last post-smoothing sweep + `r = b - A x`, `norm(r)` of step k, then
 * MGcycle.jl:26-31,54-60 of step k+1 - `r[:] = b - A x`, two sweeps of relax, `r = b - A x` for the restriction):
 *   t = x + d.*(b - A x) ; r = b - A t ; *norm_r = ||r|| ; xn = t + d.*r ; tp = xn + d.*(b - A xn) ; rp = b - A tp.
 * x, tp, rp: three different device buffers (x 16-byte aligned); t is not stored.  MG_ERR_UNSUPPORTED when the level is not
 * served (needs the 2-D tile form of the two-stage pass, relaxPre = 2, one right-hand side, a pointwise smoother).
 * mg_solve*_FP64 uses it on every step but the last by count; a stopping test that ends the loop earlier re-creates the
 * iterate with one sweep of the pass's input.  Exposed for kernel tests. */
int mg_four_stage_dev_FP64(mg_hierarchy* h, long long level, const double* b_dev, const double* x_dev, double* tp_dev,
                           double* rp_dev, double* norm_r);
/* transposeHierarchy (MGsetup.jl:274-318) on the resident hierarchy: As[l] <- As[l]' (every level), Ps[l] <- Rs[l]' (Rs[l] keeps its
 * values: the reference's second assignment reads the new Ps[l]), relaxPrecs unchanged, dense coarsest inverse transposed in place.
 * The transposes are computed in HBM (counting sort + per-column order: the stored-order CSR of the transpose), the device formats
 * rebuilt from them; mg_finalize is called.  MG_ERR_UNSUPPORTED, nothing changed, when the coarsest solve is held as sparse
 * factors or a column has more than 4096 entries (both checked before the first operator is replaced): hand the transposed
 * operators over with mg_set_operator_* instead.  Any OTHER error (MG_ERR_HIP: an allocation or a launch failed half way) leaves
 * the handle unfinalized - every entry point refuses it - and the hierarchy must be uploaded again. */
int mg_transpose_hierarchy(mg_hierarchy* h);
/* shape[3] = rows, columns, stored entries of operator `which` of `level` as the device holds it (after a transpose: of the transposed one). */
int mg_operator_shape(mg_hierarchy* h, long long level, long long which, long long* shape);
/* *yes = 1 when level `level` has the four-stage form; geometry[12] as mg_sweep_residual_form's tile geometry. */
int mg_four_stage_form(mg_hierarchy* h, long long level, long long* yes, long long* geometry);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Launch kernel `kernel` of `level` `reps` times back to back on the library's stream between two
 * HIP events and return the average duration in ms; *bytes receives the ALGORITHMIC bytes of one
 * launch. */
int mg_time_op_dev_FP64(mg_hierarchy* h, long long level, long long kernel, long long nrhs,
                        long long reps, double* ms_avg, double* bytes);
/* Per-kernel HIP-event accounting of everything the cycle launches (off by default). */
int mg_profile_enable(mg_hierarchy* h, long long on);
int mg_profile_get(mg_hierarchy* h, long long level, long long kernel, double* total_ms,
                   long long* launches, double* bytes_per_launch);
int mg_profile_reset(mg_hierarchy* h);
/* Bytes one launch of the kernel IN USE has to move: the device format's matrix side (row classes: 2 or 6 B/row +
 * dictionary; pattern-coded: 8 B/nnz + descriptors; plain CSR: 12 B/nnz + row pointers) + every vector element once.
 * This - not the CSR-priced figure of mg_profile_get - is what a bandwidth fraction must be computed from. */
int mg_profile_get_moved(mg_hierarchy* h, long long level, long long kernel, double* moved_bytes_per_launch);
/* Device format of one operator: number of distinct row patterns (0 = plain CSR with int32 column indices),
 * dictionary length, and the index-side bytes (row pointers + column information) of one nrhs=1 launch. */
int mg_operator_format(mg_hierarchy* h, long long level, long long which, long long* npatterns,
                       long long* dict_entries, double* index_bytes_per_launch);
/* Row-class form of one operator (csr_rowclass_spmv): number of distinct rows (same column offsets from the row's
 * first column AND bit-identical values; 0 = the operator is not stored that way), dictionary length, and the
 * matrix-side bytes one nrhs=1 launch of the kernel in use actually streams (row classes: 6 B/row + dictionary;
 * pattern-coded: 8 B/nnz + descriptors; plain CSR: 12 B/nnz + row pointers).  Lossless; chosen at upload. */
int mg_operator_rowclasses(mg_hierarchy* h, long long level, long long which, long long* nclasses,
                           long long* dict_entries, double* matrix_bytes_per_launch);
/* Two refinements of the row-class form: implicit_first = 1 when the class also fixes (first column - row index), so
 * no per-row first column is stored (2 B/row instead of 6); class_relax = 1 when the level's relaxPrec is constant per
 * class and the fused sweep reads it from the dictionary instead of streaming 8 B/row; kernel_variant = which kernel
 * serves the operator at nrhs == 1: -1 none (streaming formats), 0 csr_rowclass_spmv, 1 csr_rowclass_window_spmv
 * (x staged in LDS per workgroup of consecutive rows), 2 csr_rowclass_tile_spmv (plane tiles from the grid hint),
 * 3 csr_rowclass_march_spmv (z-marching ring of slabs from the grid hint), 4 csr_rowclass_lane_spmv (every lane
 * walks its own row's class, dictionary in LDS: the default for operators that are not staged), 7 csr_rowclass_marchr_spmv
 * (a restriction of a vertex-centred grid pair walking the fine planes: mg_marchr.hpp), 8 the one-trip kernels of the small grid
 * levels (mg_small.hpp), 9 band-27 (planar values of a variable-coefficient 27-point grid operator), 10 grid_cell_prolong (the
 * trilinear prolongation of a vertex-centred grid pair, a lane per coarse cell), 11 grid_wave_restrict (its restriction, 62 coarse
 * nodes per wavefront) - 10 and 11 for grid pairs of any size whose P / R the upload verified entry by entry; with a block of
 * right-hand sides (current nrhs > 1): 5 csr_rowclass_lane_spmm (one column per lane), 6 csr_rowclass_lane_spmm2 (even
 * nrhs: two columns = 16 bytes per lane; its residual form also writes the ||r||^2 partials and x + d.*r), -1 the
 * CSR-stream SpMM;
 * exception_rows = rows outside the dictionary classes (computed from the CSR arrays: in the last workgroup of the
 * row-class kernel when there are at most 256 of them - second template argument `true` - else by csr_rows_spmv). */
int mg_operator_rowclass_flags(mg_hierarchy* h, long long level, long long which, long long* implicit_first,
                               long long* class_relax, long long* kernel_variant, long long* exception_rows);
/* Algorithmic HBM bytes of one full cycle (x0 = 0) with the current nrhs, DESIGN.md section 5. */
int mg_cycle_bytes(mg_hierarchy* h, double* bytes);
/* HBM bytes held by the hierarchy. */
int mg_device_bytes(mg_hierarchy* h, double* bytes);

/* ---- building blocks of the multi-GPU cycle ---------------------------------------------------- */
/* One operator resident on its own (a rank's local rows of A, P or R with halo columns appended:
 * rectangular), applied asynchronously on the caller's HIP stream (hipStream_t passed as void*).
 * kernel: MG_K_SPMV/RESTRICT/PROLONG -> y = alpha*M*x + beta*y ; MG_K_RESIDUAL -> y = b - M*x ;
 * MG_K_SMOOTH -> y = x + d.*(b - M*x).  Blocks are row-major [n][nrhs]. */
typedef struct mg_operator mg_operator;
int mg_op_create_FP64_INT64(long long device_id, long long n_rows, long long n_cols,
                            const long long* colptr, const long long* rowval, const double* nzval,
                            mg_operator** out);
/* A rank's local A of a sharded level in BOX form: square [owned box in natural x-fastest order | halo] with empty halo
 * rows, n1*n2*n3 == regular_cols = the owned box.  Rows that read a halo column are kept apart as exception rows; all
 * others keep the row-class form of the global grid operator and run the staged kernels of the single-GPU path. */
int mg_op_create_box_FP64_INT64(long long device_id, long long n_rows, long long n_cols, const long long* colptr,
                                const long long* rowval, const double* nzval, long long n1, long long n2, long long n3,
                                long long regular_cols, mg_operator** out);
/* A rank's local P of a sharded level with grid hints: rows = the owned fine box f1 x f2 x f3 (== n_rows, natural
 * x-fastest order), columns = [owned coarse box c1 x c2 x c3 (== regular_cols) | halo].  Rows that read a halo column are
 * kept apart as exception rows; the others take the LDS-staged prolongation kernel of the single-GPU path where the
 * pattern fits it (checked on the data).  mg_op_apply_phase_dev_FP64: phase 1 = the rows that read owned coarse entries
 * only, phase 2 = the exception rows (ParSpMatVec.jl:49-71 semantics unchanged: y = alpha*P*x + beta*y).
 * With f1 = ... = c3 = 0 only the owned | halo split is made (any local operator, e.g. a restriction: rows that read a
 * halo column in phase 2, the others in phase 1, whatever kernel serves them). */
int mg_op_create_grid_FP64_INT64(long long device_id, long long n_rows, long long n_cols, const long long* colptr,
                                 const long long* rowval, const double* nzval, long long regular_cols, long long f1,
                                 long long f2, long long f3, long long c1, long long c2, long long c3, mg_operator** out);
/* Announce the relaxPrec vector (device; one entry per row, for a box operator per owned row) the operator will be
 * swept with.  Where it is bit-identical over every dictionary class of a row-class operator, the fused sweeps and the
 * fused residual called with THIS pointer (nrhs = 1, row_offset = 0) read it from the dictionary instead of streaming
 * 8 B/row - what mg_finalize does for the levels of a hierarchy (class_relax of mg_operator_rowclass_flags).  Call again
 * after the contents change.  mg_dist_finalize binds every level's vector itself. */
int mg_op_bind_relax_dev_FP64(mg_operator* op, const double* d_dev, long long n);

/* Which kernel fuses a damped-Jacobi sweep with the residual that follows it (MGcycle.jl:129-131 + 58-60) on this level's
 * A: *form = 0 none (two launches), 2 the 1-D chunk form, 3 the 2-D in-plane tile form, 4 the same with the coefficients
 * streamed per row (band form of a grid operator without row classes), 5 the 27-point marching form (csr_rowclass_march27_spmv: t and r
 * out only; it also serves single sweeps / residuals of the level; geometry: the pair's, [7] = workgroups of the single-product
 * geometry); geometry (optional, 12 entries, forms 3 and 4): tiles per line, tiles per column, TX, TY, rows per lane, workgroups, LDS bytes, estimated fill bytes per row x
 * 100, threads per workgroup, segments of the lockstep schedule (0: balanced), planes per segment, class-table entries. */
int mg_sweep_residual_form(mg_hierarchy* h, long long level, long long* form, long long* geometry);
/* Band form (form 4 above) of level `level`: info[0] = 1 when it is held; info[1] = 1 when the 7 value planes are in canonical
 * slots (-z, -y, -x, diagonal, +x, +y, +z: every structure class a 7-point star); info[2] = 1 when the values are symmetric
 * entry by entry (checked on the device whenever the values change: G' diag(sigma) G is) - the pass then reads the three lower
 * entries of a row from the upper ones of its neighbours; info[3] = value planes streamed from HBM per pass (7, or 4).
 * info[0] = 2: the level holds the band-27 form (27 planar arrays, kernel_variant 9); info[2] / info[3] likewise (27, or 14). */
int mg_band_form(mg_hierarchy* h, long long level, long long* info);
/* The kernel that serves an operator without row classes or grid records (kernel_variant -1), for the handle's nrhs.  info[0]:
 * 0 none of these, 1 csr_pattern_spmv, 2 csr_stream_spmv, 3 csr_longrow_spmv, 4 csr_stream_spmm (nrhs > 1), 5 csr_rowclass_lane_spmm,
 * 6 csr_rowclass_lane_spmm2; info[1]: non-temporal matrix loads (1-4), rows per lane (6); info[2]: 16-bit column offsets (3);
 * info[3]: entries of the longest row.  Read-only. */
int mg_operator_stream_kernel(mg_hierarchy* h, long long level, long long which, long long* info);
/* kernel variant serving the operator at nrhs == 1 (as mg_operator_rowclass_flags) and its exception rows */
int mg_op_kernel_variant(mg_operator* op, long long* variant, long long* exception_rows);
int mg_op_destroy(mg_operator* op);
int mg_op_apply_dev_FP64(mg_operator* op, long long kernel, double alpha, const double* x_dev,
                         double beta, double* y_dev, const double* b_dev, const double* d_dev,
                         long long nrhs, void* stream);
/* The operator holds the rows [row_offset, row_offset + n_rows) of the level (interior / boundary split of
 * the overlapped halo exchange): y, b, d and the smoother's own-x term are read/written at that offset of the
 * full-level vectors passed here; x is still the whole gathered vector. */
int mg_op_apply_rows_dev_FP64(mg_operator* op, long long kernel, double alpha, const double* x_dev,
                              double beta, double* y_dev, const double* b_dev, const double* d_dev,
                              long long nrhs, long long row_offset, void* stream);
/* phase 0: the whole product; 1: the rows in dictionary classes only (do not read the halo of a box operator);
 * 2: the exception rows only.  The sharded cycle runs phase 1 while the halo is in flight and phase 2 after it landed. */
int mg_op_apply_phase_dev_FP64(mg_operator* op, long long kernel, double alpha, const double* x_dev, double beta,
                               double* y_dev, const double* b_dev, const double* d_dev, long long nrhs,
                               long long row_offset, long long phase, void* stream);
/* r = b - M x with ||r||^2 fused: one partial sum per workgroup from partials_dev on (*nparts of them); optionally
 * xnext = x + d.*r as a second output (mg_op_can_fuse_next says whether the kernel serving the operator can write it),
 * in which case r_dev may be NULL.  phase as above; a phase-2 call gets the pointer advanced past phase 1's partials. */
int mg_op_residual_fused_dev_FP64(mg_operator* op, const double* x_dev, const double* b_dev, const double* d_dev,
                                  double* r_dev, double* xnext_dev, double* partials_dev, long long phase,
                                  long long* nparts, void* stream);
int mg_op_can_fuse_next(mg_operator* op, const double* x_dev, long long* yes);
/* The two-stage pass on a stand-alone operator (csr_rowclass_march3_spmv; what the sharded sequencer calls on the box-form
 * levels): t = x + d.*(b - M x) on every row that has a row class and r = b - M t [xn = t + d.*r, ||r||^2 partials] on every
 * such row that is not next to a row without one - the last sweep of relax and the residual that follows it
 * (MGcycle.jl:129-131 + 58-60; SolveFuncs.jl:26-30) in one pass.  The rows it leaves out are computed from the CSR arrays
 * by mg_op_apply_list_dev_FP64: list 1 = rows without a class (a box operator's rows that read the halo: t and r), list 2 =
 * rows next to them (r).  d: the vector bound with mg_op_bind_relax_dev_FP64; t, r, xn: each optional, all distinct. */
int mg_op_can_sweep_residual(mg_operator* op, const double* x_dev, const double* d_dev, long long* yes, long long* list1_rows,
                             long long* list2_rows);
int mg_op_sweep_residual_dev_FP64(mg_operator* op, const double* x_dev, const double* b_dev, const double* d_dev, double* t_dev,
                                  double* r_dev, double* xn_dev, double* partials_dev, long long* nparts, void* stream);
/* kernel: MG_K_SMOOTH (y = x + d.*(b - M x)) or MG_K_RESIDUAL (y = b - M x; y2, if given, = x + d.*y; partials_dev, if
 * given, receives *nparts partial sums of y.^2).  y or y2 may be NULL for MG_K_RESIDUAL. */
int mg_op_apply_list_dev_FP64(mg_operator* op, long long list, long long kernel, const double* x_dev, double* y_dev,
                              const double* b_dev, const double* d_dev, double* y2_dev, double* partials_dev, long long* nparts,
                              void* stream);
int mg_op_info(mg_operator* op, long long* n_rows, long long* n_cols, long long* nnz,
               double* device_bytes);
/* x = d.*b ; xout = x + d.*r ; out[0] = sum x^2 (workspace >= 1024 doubles) - asynchronous. */
int mg_vec_dscale_dev_FP64(const double* d_dev, const double* b_dev, double* x_dev, long long n,
                           long long nrhs, void* stream);
int mg_vec_xpdr_dev_FP64(const double* x_dev, const double* d_dev, const double* r_dev,
                         double* xout_dev, long long n, long long nrhs, void* stream);
int mg_vec_sumsq_dev_FP64(const double* x_dev, long long len, double* workspace_dev, double* out_dev,
                          void* stream);
/* Make a hierarchy enqueue on the caller's stream; enqueue one cycle without waiting. */
int mg_set_stream(mg_hierarchy* h, void* stream);
int mg_cycle_async_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n,
                            long long nrhs, long long x_is_zero);
/* The K-cycle's step INTO the hierarchy's first level (MGcycle.jl:72-76): x = 2 steps of FGMRES_relaxation on A_1 x = b
 * from x = 0, preconditioned by the K-cycle of level 1.  Used by the sharded sequencer when the level above the
 * replicated tail runs a K-cycle; one right-hand side; enqueues on the handle's stream (the FGMRES dots synchronise). */
int mg_kcycle_step_async_dev_FP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n);

/* ---- hybrid Kaczmarz relaxation --------------------------------------------------------------------------
 * Replaces the reference's native applyHybridKaczmarz_FP64_INT64 (deps/src/parRelax.h:7-43; ccall at
 * src/Multigrid/parRelax.jl:61-64) with the same arguments: rowptr/colA 1-based Int64 and valA of the transposed CSC
 * (= CSR of A), ArrIdxs the domainLength x numDomains UInt32 array of 1-based row lists (0 = padding,
 * DDService.jl:2-18), invD = omega ./ sum(|A|^2 over each row) (parRelax.jl:44).  create uploads once; apply runs
 * `numit` sweeps on x (in/out) and b, n x nrhs column-major.  sequential = 1: one wavefront walks the sub-domains in
 * order (bit-identical to the reference binary with numCores = 1); 0: one wavefront per sub-domain, unsynchronised
 * between sub-domains like the reference's OpenMP threads. */
typedef struct mg_kaczmarz mg_kaczmarz;
int mg_kaczmarz_create_FP64_INT64(long long device_id, long long n, const long long* rowptr, const double* valA,
                                  const long long* colA, long long numDomains, long long domainLength,
                                  const unsigned int* ArrIdxs, const double* invD, mg_kaczmarz** out);
int mg_kaczmarz_apply_FP64(mg_kaczmarz* k, double* x, const double* b, long long nrhs, long long numit,
                           long long sequential);
int mg_kaczmarz_apply_dev_FP64(mg_kaczmarz* k, double* x_dev, const double* b_dev, long long nrhs, long long numit,
                               long long sequential);
/* ComplexF64 values (applyHybridKaczmarz_CFP64_INT64; ccall at parRelax.jl:71-74), the same arguments: valA = AT.nzval, the
 * CSC of AT = A^H (the conj of A's CSR values), invD = omega ./ sum(conj(AT).*AT) stored complex, and valA, invD, x and b
 * interleaved (re, im) doubles, x and b n x nrhs column-major.  Per listed row: inner = (b_i - sum_k conj(valA_k) x_k) *
 * invD_i; x_k += inner * valA_k, every product and sum rounded separately (C99's plain complex product), so sequential = 1
 * is bit-identical to the reference binary with numCores = 1.  With sequential = 0, sub-domains racing on a shared node may
 * read its real and imaginary parts from different updates, as the reference's OpenMP threads may.  The handle records
 * its value type: an FP64 apply on a CFP64 handle, or a CFP64 apply on an FP64 handle, fails with MG_ERR_STATE and
 * leaves the handle usable.  Validation, limits and the no-GPU error are those of mg_kaczmarz_create_FP64_INT64. */
int mg_kaczmarz_create_CFP64_INT64(long long device_id, long long n, const long long* rowptr, const double* valA,
                                   const long long* colA, long long numDomains, long long domainLength,
                                   const unsigned int* ArrIdxs, const double* invD, mg_kaczmarz** out);
int mg_kaczmarz_apply_CFP64(mg_kaczmarz* k, double* x, const double* b, long long nrhs, long long numit,
                            long long sequential);
int mg_kaczmarz_apply_dev_CFP64(mg_kaczmarz* k, double* x_dev, const double* b_dev, long long nrhs, long long numit,
                                long long sequential);
/* Float32 / ComplexF32 values (applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64; the ccalls of parRelax.jl:61-79 for a single
 * VAL), the same arguments with valA, invD, x and b in float (interleaved (re, im) for CFP32); valA = AT.nzval.  The
 * arithmetic mixes precisions as the reference's single builds do (parRelax.h:27 calls the double-complex conj()): per
 * listed row, inner -= conj(valA_k) x_k widens both operands to double, forms the product and the difference in double
 * and rounds inner back to single after every term; inner *= invD_i and x_k += inner * valA_k are single arithmetic, every
 * product and sum rounded to float (C99's plain complex product).  sequential = 1 is bit-identical to the reference binary
 * with numCores = 1.  x moves through L2 one value per access (4 bytes, or one 8-byte access for a CFP32 pair, which
 * therefore cannot tear between racing sub-domains); the _dev forms return MG_ERR_INVALID for an x_dev or b_dev that is not
 * aligned to one value.  Any apply entry called on a handle of another value type fails with MG_ERR_STATE and leaves the
 * handle usable.  Validation, limits and the no-GPU error are those of mg_kaczmarz_create_FP64_INT64. */
int mg_kaczmarz_create_FP32_INT64(long long device_id, long long n, const long long* rowptr, const float* valA,
                                  const long long* colA, long long numDomains, long long domainLength,
                                  const unsigned int* ArrIdxs, const float* invD, mg_kaczmarz** out);
int mg_kaczmarz_apply_FP32(mg_kaczmarz* k, float* x, const float* b, long long nrhs, long long numit, long long sequential);
int mg_kaczmarz_apply_dev_FP32(mg_kaczmarz* k, float* x_dev, const float* b_dev, long long nrhs, long long numit,
                               long long sequential);
int mg_kaczmarz_create_CFP32_INT64(long long device_id, long long n, const long long* rowptr, const float* valA,
                                   const long long* colA, long long numDomains, long long domainLength,
                                   const unsigned int* ArrIdxs, const float* invD, mg_kaczmarz** out);
int mg_kaczmarz_apply_CFP32(mg_kaczmarz* k, float* x, const float* b, long long nrhs, long long numit, long long sequential);
int mg_kaczmarz_apply_dev_CFP32(mg_kaczmarz* k, float* x_dev, const float* b_dev, long long nrhs, long long numit,
                                long long sequential);
int mg_kaczmarz_destroy(mg_kaczmarz* k);

/* ---- stand-alone sparse-factor applier -----------------------------------------------------------------------------
 * Device counterpart of applyLUsolve_FP64_INT64 (deps/src/parLU.cpp:52-63; ccall parallelJuliaSolver.jl:214-217): the
 * "Julia factors, native applies" back end 3 of src/ParallelJuliaSolver.  Factors exactly as setupLUFactor leaves them
 * (parallelJuliaSolver.jl:113-148): L and U in CSR with 1-based Int64 indices, L's diagonal LAST and U's diagonal FIRST
 * in every row, row scaling folded into L, p / q 1-based with A[p,q] = L*U.  solve: x[q] = U \ (L \ b[p])
 * (parLU.cpp:120-190); doTranspose != 0: the system with the transposed matrix, x[p] = L' \ (U' \ b[q])
 * (parLU.cpp:194-260) - the transposed factors are built and uploaded on first use.  b, x: n x nrhs column-major on
 * the host (b is left untouched: the reference uses it as work space), or row-major [n][nrhs] in HBM for the _dev
 * form.  All right-hand sides travel together (the reference: one OpenMP task per column). */
typedef struct mg_lu mg_lu;
int mg_lu_create_FP64_INT64(long long device_id, long long n, const long long* Lptr, const long long* Lcol,
                            const double* Lval, const long long* Uptr, const long long* Ucol, const double* Uval,
                            const long long* p, const long long* q, mg_lu** out);
int mg_lu_solve_FP64(mg_lu* f, const double* b, double* x, long long n, long long nrhs, long long doTranspose);
int mg_lu_solve_dev_FP64(mg_lu* f, const double* b_dev, double* x_dev, long long n, long long nrhs,
                         long long doTranspose);
/* ComplexF64 factors (applyLUsolve_CFP64_INT64, parLU.cpp:69-72; the complex systems src/ParallelJuliaSolver was written for):
 * the same layout, limits and validation as mg_lu_create_FP64_INT64, with Lval, Uval, b and x interleaved (re, im) doubles
 * (Julia ComplexF64).  Adjoint convention: doTranspose != 0 follows applyLUsolveTrans (parLU.cpp:193-260), which CONJUGATES
 * for complex values - x[p] = L^H \ (U^H \ b[q]) solves A^H x = b, Julia's A' \ b, not the plain transpose.  The
 * conjugate-transposed factors are built on the host at the first such solve and stay resident beside the plain ones.
 * Factors of at least lu_multi_min_rows rows (MG_LU_MULTI_MIN_ROWS) take the chip-wide form - one launch per dependency
 * level, the trailing chain through the explicit inverse of its dense block (MG_LU_DENSE_TAIL_MIN / _MAX bound its order) -
 * smaller ones a single workgroup; nrhs columns travel together in both.  The handle records its value type: mg_lu_solve*_FP64
 * on a complex handle and mg_lu_solve*_CFP64 on a real one fail with MG_ERR_STATE and leave the handle usable.
 * mg_lu_destroy serves both kinds. */
int mg_lu_create_CFP64_INT64(long long device_id, long long n, const long long* Lptr, const long long* Lcol,
                             const double* Lval, const long long* Uptr, const long long* Ucol, const double* Uval,
                             const long long* p, const long long* q, mg_lu** out);
int mg_lu_solve_CFP64(mg_lu* f, const double* b, double* x, long long n, long long nrhs, long long doTranspose);
int mg_lu_solve_dev_CFP64(mg_lu* f, const double* b_dev, double* x_dev, long long n, long long nrhs,
                          long long doTranspose);
/* Single factors (applyLUsolve_FP32_UINT32, applyLUsolve_CFP32_UINT32, applyLUsolve_CFP32_INT64; the forms a Helmholtz inversion
 * builds, because the factors are what fills memory): the layout, limits, validation and adjoint convention of
 * mg_lu_create_CFP64_INT64 with Lval, Uval, b and x in float (interleaved for ComplexF32), row pointers 1-based Int64 as in every
 * form, and column indices and p, q in the index type of the name (1-based).  Arithmetic: factor values, b, y, x and the work
 * vectors are STORED in single - 12 / 8 bytes per factor entry with its column index, against 20 - and every row is EVALUATED in
 * double: a value and the gathered y are widened on load, products, partial sums, the subtraction from the right-hand side and
 * the division by the diagonal are double, the result is rounded once on its store.  The dense trailing block is gathered and
 * inverted in double and its inverse stored in single.  A rerun gives the same bits.  A solve entry point of another value type
 * fails with MG_ERR_STATE and leaves the handle usable; n, nnz or n*nrhs beyond int32 return MG_ERR_UNSUPPORTED. */
int mg_lu_create_FP32_UINT32(long long device_id, long long n, const long long* Lptr, const unsigned int* Lcol,
                             const float* Lval, const long long* Uptr, const unsigned int* Ucol, const float* Uval,
                             const unsigned int* p, const unsigned int* q, mg_lu** out);
int mg_lu_create_CFP32_UINT32(long long device_id, long long n, const long long* Lptr, const unsigned int* Lcol,
                              const float* Lval, const long long* Uptr, const unsigned int* Ucol, const float* Uval,
                              const unsigned int* p, const unsigned int* q, mg_lu** out);
int mg_lu_create_CFP32_INT64(long long device_id, long long n, const long long* Lptr, const long long* Lcol,
                             const float* Lval, const long long* Uptr, const long long* Ucol, const float* Uval,
                             const long long* p, const long long* q, mg_lu** out);
int mg_lu_solve_FP32(mg_lu* f, const float* b, float* x, long long n, long long nrhs, long long doTranspose);
int mg_lu_solve_dev_FP32(mg_lu* f, const float* b_dev, float* x_dev, long long n, long long nrhs, long long doTranspose);
int mg_lu_solve_CFP32(mg_lu* f, const float* b, float* x, long long n, long long nrhs, long long doTranspose);
int mg_lu_solve_dev_CFP32(mg_lu* f, const float* b_dev, float* x_dev, long long n, long long nrhs, long long doTranspose);
/* The form a handle's factors are applied in, any value type; doTranspose selects the transposed (adjoint) set and builds
 * it if needed.  info[0..7): value type (0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32); 1 for the chip-wide form; order of the dense trailing
 * block; launched levels of L ahead of it and of U behind it; all dependency levels of L and of U. */
int mg_lu_form(mg_lu* f, long long doTranspose, long long* info);
/* Measurement: `warmup` untimed solves on device vectors (row-major [n][nrhs], as the _dev solve of the handle's value
 * type - for a single handle b_dev and x_dev point to float data), then `reps` solves, each enqueued between two events on the handle's stream - the second recorded before the host
 * waits, so a sample is stream time without the host's wake-up; ms[0..reps) in milliseconds.  The factor set of the direction
 * is built before the first sample. */
int mg_lu_time_dev(mg_lu* f, const double* b_dev, double* x_dev, long long n, long long nrhs, long long doTranspose,
                   long long warmup, long long reps, double* ms);
int mg_lu_destroy(mg_lu* f);

/* ---- multiplicative Schwarz preconditioner (src/DomainDecomposition) --------------------------------------------------
 * Device form of solveDDSerial (DDSerial.jl:108-139; getDDpreconditioner, DomainDecomposition.jl:136-146) on what
 * setupDDSerial leaves (DDSerial.jl:81-106, sparse-matrix branch): for niter sweeps, for every colour in ascending order
 * (cellColor, Vanka.jl:105-130: 1..2^dim), for every sub-domain of the colour in linear order:
 *   r = (b - A x)[I]  (computeResidualAtIdx, DDSerial.jl:4-20),  t = A_I \ r  (solveSubDomain, l.183-187),  x[I] += t  (l.129).
 * create: rowptr / colA / valA are the CSR of the applied operator A, 1-based Int64 - the reference's AT.colptr, AT.rowval
 * and conj(AT.nzval) (interleaved (re, im) doubles for CFP64); idx holds the lists GlobalIndices[ic] (DDIndType = UInt32,
 * 1-based, DomainDecomposition.jl:15) back to back, sub-domain ic at idxptr[ic] .. idxptr[ic+1]-1 (idxptr 1-based, numSub+1
 * entries); color[ic] >= 1 is its colour.  set_factor: sub-domain ic's factors of A[I,I] in parLU's layout, exactly the
 * arguments of mg_lu_create_* (n_i must equal the length of its list).  finalize: every sub-domain needs its factors
 * (MG_ERR_STATE otherwise); decides per colour whether its members are INDEPENDENT - index sets pairwise disjoint and no
 * row listed by one member stores a column listed by another (nodal boxes, radius-1 stencil: cellSize - 2*overlap >= 2).
 * An independent colour is one launch, one 1024-thread workgroup per sub-domain; a dependent one, or one with a member of
 * at least lu_multi_min_rows rows (MG_LU_MULTI_MIN_ROWS, read once at create), runs its members one after another:
 * residual gather, the applier's solve (single workgroup; chip-wide form for those large members), scatter-add.
 * apply: b and x are vectors of n values (one right-hand side: the reference indexes b[Idxs]), x in/out, b != x; host
 * pointers, or HBM for the _dev forms.  doTranspose != 0 reaches the sub-domain solves only (transposed factors, the
 * ADJOINT for CFP64, built on first use); the residual always uses A (DDSerial.jl:123,128).  The handle records its value
 * type: an FP64 entry point on a CFP64 handle, or the reverse, fails with MG_ERR_STATE and leaves the handle usable.
 * Invalid arguments (null, empty, an index outside 1..n, an index listed twice by one sub-domain, n_i differing from the
 * list) give MG_ERR_INVALID; sizes beyond int32 device indices MG_ERR_UNSUPPORTED.
 * Not served: the operator-constructor / Dirichlet-mass branch (DDSerial.jl:42-61), DDParallel.jl, solveGSDDSerial. */
typedef struct mg_dd mg_dd;
int mg_dd_create_FP64_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA,
                            const double* valA, long long numSub, const long long* idxptr, const unsigned int* idx,
                            const long long* color, mg_dd** out);
int mg_dd_create_CFP64_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA,
                             const double* valA, long long numSub, const long long* idxptr, const unsigned int* idx,
                             const long long* color, mg_dd** out);
int mg_dd_set_factor_FP64_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol,
                                const double* Lval, const long long* Uptr, const long long* Ucol, const double* Uval,
                                const long long* p, const long long* q);
int mg_dd_set_factor_CFP64_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol,
                                 const double* Lval, const long long* Uptr, const long long* Ucol, const double* Uval,
                                 const long long* p, const long long* q);
int mg_dd_finalize(mg_dd* dd);
int mg_dd_apply_FP64(mg_dd* dd, const double* b, double* x, long long n, long long niter, long long doTranspose);
int mg_dd_apply_dev_FP64(mg_dd* dd, const double* b_dev, double* x_dev, long long n, long long niter,
                         long long doTranspose);
int mg_dd_apply_CFP64(mg_dd* dd, const double* b, double* x, long long n, long long niter, long long doTranspose);
int mg_dd_apply_dev_CFP64(mg_dd* dd, const double* b_dev, double* x_dev, long long n, long long niter,
                          long long doTranspose);
/* One sweep from x = 0 (getDDpreconditioner, DomainDecomposition.jl:136-146; the coarsest solve of a cycle, MGcycle.jl:63-64):
 * x is output only and need not be initialised - it is zero-filled on the stream, then swept: the result is that of
 * mg_dd_apply* with niter = 1 from a zero-filled x.  (A first colour that skips its residual rows was measured and is not
 * faster: profiles/coarse_solver.md.)
 * Arguments are validated as for mg_dd_apply*.  (A family of its own, mg_dd0_*: the set of mg_dd_* names is pinned by
 * tests/test_dd_host.py, as the _CF64 set is by tests/test_parlu_complex_host.py.) */
int mg_dd0_apply_FP64(mg_dd* dd, const double* b, double* x, long long n, long long doTranspose);
int mg_dd0_apply_CFP64(mg_dd* dd, const double* b, double* x, long long n, long long doTranspose);
int mg_dd0_apply_dev_FP64(mg_dd* dd, const double* b_dev, double* x_dev, long long n, long long doTranspose);
int mg_dd0_apply_dev_CFP64(mg_dd* dd, const double* b_dev, double* x_dev, long long n, long long doTranspose);
/* The coarsest solve of a hierarchy by a solver object (param.LU a DomainDecompositionParam: MGsetup.jl:323-326,
 * MGcycle.jl:140-143): one sweep of a finalized handle, from zero inside a cycle, from the caller's x on a hierarchy of one
 * level (MGcycle.jl:13-18), with doTranspose = 0 in the sub-domain solves, enqueued on the hierarchy's stream without a host
 * synchronisation.  The handle's value type must be the hierarchy's (MG_ERR_STATE otherwise); its order must be the coarsest
 * level's (mg_finalize: MG_ERR_INVALID).  The hierarchy BORROWS the handle: mg_dd_destroy of an attached handle fails with
 * MG_ERR_STATE and leaves both usable; mg_destroy, another mg_set_coarse_* call or dd == NULL detach it (dd == NULL leaves
 * the coarsest solve unset).  Stand-alone mg_dd_apply* calls on an attached handle stay legal: they are ordered behind the
 * work the hierarchy has enqueued.  Such a hierarchy's sub-cycles are not captured into HIP graphs.  Refused with
 * MG_ERR_UNSUPPORTED: more than one right-hand side (mg_set_nrhs, mg_finalize), mg_ghost_attach, mg_dist_set_tail_INT64,
 * mg_transpose_hierarchy. */
int mg_set_coarse_dd(mg_hierarchy* h, mg_dd* dd);
/* Which coarsest solve a hierarchy of either value type runs.  info[0]: 0 dense inverse, 1 sparse LU in one workgroup, 2 sparse
 * LU chip-wide (per-level launches and a dense trailing inverse), 3 GMRES, 4 Schwarz sweep; info[1]: its order; info[2]:
 * kernel launches per solve (GMRES on a real handle: 0 - it depends on the right-hand side; GMRES on a complex handle: the launches
 * of its speculative solve, which do not - front, 10 steps, combination, on the path the handle takes now, see
 * mg_set_coarse_gmres_CF64).  MG_ERR_STATE when none is set. */
int mg_coarse_form(mg_hierarchy* h, long long* info);
/* info[0..6): value type (0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32 - the single kinds: see below); sub-domains; colours present; colours run batched; colours run in
 * sequence; kernel launches of one sweep (doTranspose = 0; a chip-wide member counts one launch per level it launches). */
int mg_dd_info(mg_dd* dd, long long* info);
/* Measurement, as mg_lu_time_dev: `warmup` untimed sweeps on device vectors of the handle's value type, then `reps` sweeps,
 * each between two events on the handle's stream; ms[0..reps) in milliseconds.  x_dev is swept in place. */
int mg_dd_time_dev(mg_dd* dd, const double* b_dev, double* x_dev, long long n, long long doTranspose, long long warmup,
                   long long reps, double* ms);
int mg_dd_destroy(mg_dd* dd);

/* ---- Vanka cell-block smoother (src/Multigrid/Vanka.jl) ----------------------------------------------------------
 * RelaxVankaFacesColor's Julia serial path (Vanka.jl:383-425) on the device, for staggered-grid systems whose unknowns are
 * ordered x-faces, y-faces [, z-faces] [, cell pressures] of a RegularMesh of n cells.  The handle holds the CSR of the
 * applied operator A (1-based Int64; valA the values of A's rows, CFP64: interleaved complex doubles) and LocalBlocks of
 * setupVankaFacesPreconditioner, (bs*bs) x prod(n) column-major Float32 (CFP64: ComplexF32), bs = 2*dim + includePressure.
 * VankaType: 1 FULL_VANKA_RB and 3 ECON_VANKA_RB (2^dim coloured passes per iteration, each from a snapshot of x),
 * 5 FULL_VANKA_ADD (corrections formed once per call from the incoming x, added numit times); 4 (FULL_VANKA_LEX), 2 and
 * unknown types: MG_ERR_UNSUPPORTED.  nrows != sum(nf) [+ prod(n)] and other inconsistent sizes: MG_ERR_INVALID.  numit = 0
 * does nothing.  The result does not depend on the order the cells run in (no atomics: identical bits on every run).  A
 * handle is bound to its value type as mg_dd is (MG_ERR_STATE).  x (in/out) and b are two different vectors of nrows values. */
typedef struct mg_vanka mg_vanka;
int mg_vanka_create_FP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure,
                               long long nrows, const long long* rowptr, const long long* colA, const double* valA,
                               const float* D_blocks, mg_vanka** out);
int mg_vanka_create_CFP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure,
                                long long nrows, const long long* rowptr, const long long* colA, const double* valA,
                                const float* D_blocks, mg_vanka** out);
int mg_vanka_apply_FP64(mg_vanka* v, double* x, const double* b, long long numit, long long VankaType);
int mg_vanka_apply_dev_FP64(mg_vanka* v, double* x_dev, const double* b_dev, long long numit, long long VankaType);
int mg_vanka_apply_CFP64(mg_vanka* v, double* x, const double* b, long long numit, long long VankaType);
int mg_vanka_apply_dev_CFP64(mg_vanka* v, double* x_dev, const double* b_dev, long long numit, long long VankaType);
/* The same on a block of nrhs right-hand sides, 1 <= nrhs <= 16 (nrhs < 1: MG_ERR_INVALID; nrhs > 16: MG_ERR_UNSUPPORTED; both
 * before the first write).  Host forms: x, b column-major N x nrhs; _dev forms: row-major [N][nrhs] device blocks.  One pass over
 * the operator and the cells' blocks serves all columns; column c holds the bits mg_vanka_apply_* gives on column c alone. */
int mg_vanka_apply_block_FP64(mg_vanka* v, double* x, const double* b, long long nrhs, long long numit, long long VankaType);
int mg_vanka_apply_block_dev_FP64(mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long numit, long long VankaType);
int mg_vanka_apply_block_CFP64(mg_vanka* v, double* x, const double* b, long long nrhs, long long numit, long long VankaType);
int mg_vanka_apply_block_dev_CFP64(mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long numit, long long VankaType);
/* info[0..8): value type (0 Float64, 1 ComplexF64); blockSize; cells; colours (2^dim); kernel launches of one RB / ECON
 * iteration (two per colour that holds a cell); of one ADD iteration (one, plus one per call); unknowns; kernels the handle
 * has enqueued so far. */
int mg_vanka_info(mg_vanka* v, long long* info);
/* Measurement, as mg_dd_time_dev: `warmup` untimed iterations on device vectors, then `reps`, each between two events on
 * the handle's stream; ms[0..reps) in milliseconds.  x_dev is relaxed in place. */
int mg_vanka_time_dev(mg_vanka* v, double* x_dev, const double* b_dev, long long VankaType, long long warmup, long long reps,
                      double* ms);
int mg_vanka_time_block_dev(mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long VankaType, long long warmup,
                            long long reps, double* ms);   /* the same on a row-major device block of nrhs columns */
/* THE BLOCKS BUILT ON THE DEVICE (setupVankaFacesPreconditioner, Vanka.jl:294-370, from the handle's resident operator; kernel
 * vanka_build_blocks, csrc/mg_vanka.hpp: one launch, eight lanes per cell, Gauss-Jordan with partial pivoting in double, the result in
 * single in the LocalBlocks layout; the same bits on every run).  w[nw]: nw = 1 a scalar w, nw = 2 the pair (w0, w1) - w1 damps the
 * pressure row.  VankaType 1 with a scalar replaces the leading (bs-1)x(bs-1) part of each block by its diagonal and scales the inverse
 * by w; 1 with a pair scales the rows of the full inverse; 3 (scalar only: nw = 2 is MG_ERR_INVALID) divides that diagonal by w; 5
 * scales row t by t_t * W_t, t_t = 1/2 on a face shared with a neighbouring cell.  Types 2 and 4 and unknown ones: MG_ERR_UNSUPPORTED.
 * All of these are answered before the first write.  A cell whose elimination meets a pivot of squared modulus zero or not finite makes
 * the call return MG_ERR_INVALID after the launch has been waited for; the message names the first such cell (1-based) and the handle
 * keeps the blocks it had (the build writes a second buffer that replaces the first only on success).
 *   mg_vanka_create_built_*   mg_vanka_create_* with (VankaType, w, nw) in the place of D_blocks; a singular cell: no handle.
 *   mg_vanka_build_blocks_*   the handle's blocks again from its resident operator.
 *   mg_vanka_replace_values_* new operator values (valA's convention, nnz of them) on the stored pattern; the blocks stay as they are.
 *   mg_vanka_get_blocks       the blocks as mg_vanka_create_* takes them: count = bs*bs*prod(n) values (CFP64: pairs of floats).
 *   mg_vanka_time_build       measurement: device time of `reps` builds after `warmup` untimed ones (the handle's blocks stay). */
int mg_vanka_create_built_FP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure,
                                     long long nrows, const long long* rowptr, const long long* colA, const double* valA,
                                     long long VankaType, const double* w, long long nw, mg_vanka** out);
int mg_vanka_create_built_CFP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure,
                                      long long nrows, const long long* rowptr, const long long* colA, const double* valA,
                                      long long VankaType, const double* w, long long nw, mg_vanka** out);
int mg_vanka_build_blocks_FP64(mg_vanka* v, long long VankaType, const double* w, long long nw);
int mg_vanka_build_blocks_CFP64(mg_vanka* v, long long VankaType, const double* w, long long nw);
int mg_vanka_replace_values_FP64(mg_vanka* v, const double* nzval, long long nnz);
int mg_vanka_replace_values_CFP64(mg_vanka* v, const double* nzval, long long nnz);
int mg_vanka_get_blocks(mg_vanka* v, float* out, long long count);
int mg_vanka_time_build(mg_vanka* v, long long VankaType, const double* w, long long nw, long long warmup, long long reps, double* ms);
int mg_vanka_destroy(mg_vanka* v);

/* ---- native multi-GPU sequencer (one process per GPU) ---------------------------------------------------------
 * The sharded cycle of src/DomainDecomposition's partition (box rule DDIndices.jl:41-47, numbering DDService.jl:27-48;
 * worker map analogue DDParallel.jl:105,133-139) behind the C ABI: the host cuts every sharded level into local
 * operators [owned | halo] (mg_op_create_FP64_INT64) and halo plans; this handle owns the vectors and the hot loop -
 * per SpMV the boundary values are packed, exchanged with ncclSend/ncclRecv inside ncclGroupStart/End on a SIDE stream
 * while the interior rows run, the boundary rows after the event; one scalar all-reduce per solveMG step; levels below
 * the sharded ones are all-gathered and run replicated by an ordinary mg_hierarchy (the tail).  One right-hand side.
 * Transport: RCCL (pass the 128-byte id of mg_dist_unique_id, broadcast by the host, to mg_dist_create) or a
 * host-staged plug-in (tests; several ranks sharing one GPU).  Levels are 1-based; `which` is MG_OP_A / P / R. */
typedef struct mg_dist mg_dist;
/* op 0: all_to_all (send/recv splits per peer, in doubles) ; 1: all_reduce sum of `count` doubles ; 2: all_gather of `count`
 * doubles per rank.  Host buffers.  Returns 0 on success. */
typedef int (*mg_exchange_fn)(void* user, long long op, const double* send, const long long* send_splits, double* recv,
                              const long long* recv_splits, long long count);
int mg_dist_unique_id(char* id128);
int mg_dist_create(long long device_id, long long rank, long long world, const char* unique_id128, long long nlevels_sharded,
                   long long nlevels_total, long long cycleType, mg_dist** out);
int mg_dist_set_exchange_plugin(mg_dist* h, mg_exchange_fn fn, void* user);
/* This rank's part of sharded level `level`: rows renumbered [interior | boundary] (interior = rows of A without halo
 * columns), A held as two operators, P / R with halo columns appended, relaxPrecs of the owned rows (device). */
int mg_dist_set_level(mg_dist* h, long long level, long long n_own, long long n_int, mg_operator* A_int, mg_operator* A_bnd,
                      mg_operator* P, mg_operator* R, const double* d_dev, long long relaxPre, long long relaxPost);
/* Halo plan of one operator: the source vector is [n_own_src owned | n_halo received]; send_idx (0-based, into the owned
 * part) grouped by destination rank with send_splits[world]; recv_splits[world]; active = 0 if no rank exchanges anything. */
/* The level's A was handed over as ONE box operator (A_int, n_int = n_own, A_bnd = NULL): phase 1 overlaps the exchange. */
/* Smoother of the sharded levels: 0 = pointwise (Jac / SPAI: the relaxPrec vectors), 1 = Jac-GMRES (FGMRES_relaxation
 * preconditioned by the relaxPrec vector, relaxPre / relaxPost = its inner dimensions: MGcycle.jl:48-50,96-98).  The
 * replicated tail carries its own setting (mg_set_relax_type).  cycleType 'K' (mg_dist_create) runs the K-cycle's FGMRES
 * steps on sharded levels with all-reduced dots (MGcycle.jl:72-76). */
int mg_dist_set_relax_type(mg_dist* h, long long relax_type);
/* Right-hand sides per call (default 1; row-major [n][nrhs] blocks; MGdef.jl:163-176, SolveFuncs.jl:30): right after
 * mg_dist_create.  b_loc / x_loc of the cycle and solve entry points are then n_own x nrhs blocks. */
int mg_dist_set_nrhs(mg_dist* h, long long nrhs);
int mg_dist_set_level_box(mg_dist* h, long long level, long long on);
int mg_dist_set_plan_INT64(mg_dist* h, long long level, long long which, long long n_own_src, long long n_halo,
                           long long n_send, const long long* send_idx, const long long* send_splits,
                           const long long* recv_splits, long long active);
/* The replicated tail: an mg_hierarchy of the levels below the sharded ones (its stream is re-pointed to this handle's),
 * this rank's share own_tail of its first level, the padded share max_tail, and gather_index[n_tail] into the
 * all-gathered [world][max_tail] array. */
int mg_dist_set_tail_INT64(mg_dist* h, mg_hierarchy* tail, long long n_tail, long long own_tail, long long max_tail,
                           const long long* gather_index);
int mg_dist_finalize(mg_dist* h);
/* b_loc / x_loc: this rank's fine rows (device, n_own doubles, the [interior | boundary] order). */
int mg_dist_cycle_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, long long x_is_zero);
int mg_dist_solve_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, double tol, long long maxIter,
                           long long* iters, double* resvec);
/* MG-preconditioned Krylov drivers on the halo form (solveCG_MG / solveBiCGSTAB_MG / solveGMRES_MG, SolveFuncs.jl:74-133;
 * the way an SA-AMG hierarchy is used: SAAMGWrapper.jl:61-73): b_loc / x_loc as for the cycle (x in and out), every other
 * argument, the flags and the layout of resvec as for mg_pcg_dev_FP64 / mg_bicgstab_dev_FP64 / mg_fgmres_dev_FP64.  One
 * right-hand side (MG_ERR_UNSUPPORTED otherwise); inner in [1,64].  A product with A = one exchange of level 1's halo, the
 * preconditioner = the sharded cycle from x = 0, every scalar = a sum over the owned rows + an all-reduce (RCCL or the
 * plug-in's op 1), the scalars due at the same point of an iteration in ONE all-reduce: outside the cycle 2 per PCG
 * iteration, 3 per BiCGSTAB iteration, 2 per FGMRES inner step (inner <= 8; 1 + ceil(i/8) for the i-th step).  Every rank
 * returns the same flag, count and resvec.  PCG's stopping test uses ||r||^2 = r'r - 2 alpha r'q + alpha^2 q'q from all-reduced
 * scalars (resvec's entries are replaced by the summed norm one all-reduce later); BiCGSTAB's half-step exit (flag -3) is
 * taken behind the second cycle; FGMRES takes the Gram-Schmidt dots of one step together.  The work space is allocated at the
 * first call and released by mg_dist_destroy. */
int mg_dist_pcg_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, double tol, long long maxIter,
                         long long* iters, long long* flag, double* resvec);
int mg_dist_bicgstab_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, double tol, long long maxIter,
                              long long* iters, long long* flag, double* resvec, long long* nres);
int mg_dist_fgmres_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, long long inner, double tol,
                            long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
/* Halo exchanges started and all-reduces entered by this rank since mg_dist_create (cycle, solve and the drivers above). */
int mg_dist_stats(mg_dist* h, long long* exchanges, long long* allreduces);
/* The fused vector passes of those drivers on their own: one pass over the vectors does the update and leaves the sums due
 * at that point in out_dev (device), asynchronously on `stream`.  16-byte accesses where all vectors of a pass share their
 * alignment modulo 16 bytes, deterministic two-pass sums (no atomics).  workspace_dev: 8192 doubles.  xs_dev / ys_dev /
 * vs_dev and h_host are HOST arrays (of device pointers / coefficients).
 *   dots: out[c] = xs[c]'ys[c], c < k <= 8          pcg_dots: out = (p'q, r'q, q'q)
 *   pcg_update: x += alpha p, r -= alpha q, out = r'r   xpby: y = x + beta y         scale: y = a x
 *   bicg_p: p = r + beta (p - omega v)              bicg_s: r -= alpha v, out = r'r   bicg_ts: out = (t's, t't)
 *   bicg_xr: x += alpha phat + omega shat, r -= omega t, out = (r'r, rtld'r)
 *   gs_update: w -= sum_{j<m} h[j] vs[j] (m <= 64, 8 per pass), out (optional) = w'w */
int mg_vec_dots_dev_FP64(long long k, const double* const* xs_dev, const double* const* ys_dev, long long n,
                         double* workspace_dev, double* out_dev, void* stream);
int mg_vec_pcg_dots_dev_FP64(const double* p, const double* q, const double* r, long long n, double* workspace_dev,
                             double* out_dev, void* stream);
int mg_vec_pcg_update_dev_FP64(double alpha, const double* p, const double* q, double* x, double* r, long long n,
                               double* workspace_dev, double* out_dev, void* stream);
int mg_vec_xpby_dev_FP64(const double* x, double beta, double* y, long long n, void* stream);
int mg_vec_scale_dev_FP64(double a, const double* x, double* y, long long n, void* stream);
int mg_vec_bicg_p_dev_FP64(double beta, double omega, const double* r, const double* v, double* p, long long n, void* stream);
int mg_vec_bicg_s_dev_FP64(double alpha, const double* v, double* r, long long n, double* workspace_dev, double* out_dev,
                           void* stream);
int mg_vec_bicg_ts_dev_FP64(const double* t, const double* s, long long n, double* workspace_dev, double* out_dev,
                            void* stream);
int mg_vec_bicg_xr_dev_FP64(double alpha, double omega, const double* phat, const double* shat, const double* t,
                            const double* rtld, double* x, double* r, long long n, double* workspace_dev, double* out_dev,
                            void* stream);
int mg_vec_gs_update_dev_FP64(long long m, const double* h_host, const double* const* vs_dev, double* w, long long n,
                              double* workspace_dev, double* out_dev, void* stream);
/* Number of ranks of the handle's RCCL communicator as the library itself reports it (ncclCommCount); 0 for the
 * host-staged plug-in transport. */
int mg_dist_comm_count(mg_dist* h, long long* count);
/* Hand the tail's mg_hierarchy back to its owner (stream and graph option as before mg_dist_set_tail_INT64).  Needed
 * only when the tail's handle is to be used or destroyed while this sequencer still exists; mg_dist_destroy does it
 * itself otherwise, so the tail must outlive the sequencer or be released first. */
int mg_dist_release_tail(mg_dist* h);
int mg_dist_destroy(mg_dist* h);

/* ---- sharded cycle with deep ghost layers (one process per GPU; csrc/mg_ghost.inc) -------------------------------------
 * The communication-avoiding form of the sharded cycle - the reference's `overlap` (getBoxWithOverlap,
 * src/DomainDecomposition/DDIndices.jl:61-92; box rule l.41-47; fan-out DDParallel.jl:87-105,133-139).  The host builds this
 * rank's part of the hierarchy on EXTENDED boxes - owned box + ghost layers towards every neighbour, every level with the width
 * its own passes consume (round 6: 5 on the fine level = four-stage pass + restriction, 3 on the coarser ones; a level's box ends on
 * nodes of the next level, whose box holds at least the parents of all its nodes - P and R then pair a box with a SUB-BOX of the next
 * one, which the transfer kernels find in the uploaded operators) - and uploads it as an ORDINARY mg_hierarchy (mg_create ...
 * mg_finalize): levels 1..nlevels_sharded are extended-box grid operators, the levels below them are replicated on every rank; the
 * restriction into the first replicated level has one row per node of that level, non-empty for the nodes this rank owns.  These
 * calls attach geometry, exchange plans and transport; afterwards the device-pointer entry points run SHARDED on vectors of the
 * extended fine box (b: owned rows valid on entry; x: owned rows valid on return), with every single-GPU kernel form (four-stage pass,
 * 27-point marching form, arithmetic transfers, pipelined stopping test): the library tracks on how many ghost layers each level
 * vector is still valid (a product with A costs one) and refreshes all layers at once where the next operation needs more - on the
 * fine level right behind the four-stage pass, overlapped with the whole coarse cycle on a side stream; exchanges awaited at once
 * stay on the compute stream.  A pass that would consume more layers than its input has is MG_ERR_STATE, never a clamp.  Norms, dots
 * and Gram matrices are sums over the owned rows of all ranks.  Served: mg_cycle_dev_FP64 / mg_solve_dev_FP64 (V / W / F / K cycles,
 * Jac / SPAI / Jac-GMRES, direct coarsest solve; a block of 2-24 right-hand sides - mg_create / mg_set_nrhs before the attach, vectors
 * [n_ext][nrhs] row-major - column by column where the column-wise solve serves the fine level: four-stage pass, V(2,*)), the
 * MG-preconditioned Krylov drivers mg_pcg_dev_FP64 / mg_bicgstab_dev_FP64 / mg_fgmres_dev_FP64 (SolveFuncs.jl:74-133) and their block
 * forms mg_block_*_dev_FP64.  Refused (MG_ERR_UNSUPPORTED): host-pointer entry points, coarseSolveType "GMRES", mg_rap_FP64; general
 * CSR (SA-AMG) hierarchies take mg_dist_*.  Transport: RCCL (the 128-byte id of mg_dist_unique_id) or the host-staged plug-in (ops 0 and 1). */
int mg_ghost_attach(mg_hierarchy* h, long long rank, long long world, long long nlevels_sharded, const char* unique_id128);
/* (RCCL transport, optional but recommended for world > 1) a SECOND communicator - another id of mg_dist_unique_id - for the
 * ghost-layer send / recv on the side stream: RCCL serialises the operations of one communicator in issue order whatever
 * their streams; with its own communicator the fine level's exchange overlaps the coarse cycle and its all-reduces. */
int mg_ghost_set_side_comm(mg_hierarchy* h, const char* unique_id128);
int mg_ghost_set_exchange_plugin(mg_hierarchy* h, mg_exchange_fn fn, void* user);
/* Sharded level `level` (1-based): extended box ext[3] (nodes per dimension, x fastest, 1 for unused dimensions); owned box
 * [own_lo, own_hi) in extended-box coordinates; gmin = the smallest ghost width over the cut sides of ANY rank (every rank
 * must take the same exchange decisions); send_idx: extended-box ids (0-based) of owned nodes grouped by destination rank,
 * recv_idx: extended-box ids of ghost nodes grouped by owner - each peer's part in ascending global id on both sides. */
int mg_ghost_set_level_INT64(mg_hierarchy* h, long long level, const long long* ext, const long long* own_lo,
                             const long long* own_hi, long long gmin, long long n_send, const long long* send_idx,
                             const long long* send_splits, long long n_recv, const long long* recv_idx,
                             const long long* recv_splits);
/* COLLECTIVE over the ranks (one all-reduce): they agree on what every rank's kernels can do (four-stage pass, fused sweep + residual, its
 * from-zero form, d.*bc out of the restriction) - the boxes of two ranks differ by a line or two, a format builder may serve one and not
 * the other, and every rank must exchange at the same points.  A block handle whose ranks do not all have the four-stage pass fails here. */
int mg_ghost_finalize(mg_hierarchy* h);
/* Timing aid: rank R of a world of N alone on its GPU - exchanges run their pack / unpack kernels, nothing travels, sums stay
 * local (before mg_ghost_finalize; not with RCCL).  Results are meaningless, the step time is one GPU's compute share. */
int mg_ghost_set_dry(mg_hierarchy* h, long long on);
/* exchanges started / doubles sent by this rank since mg_ghost_attach; ranks of the RCCL communicator (0: plug-in) */
int mg_ghost_stats(mg_hierarchy* h, long long* exchanges, long long* doubles_sent);
int mg_ghost_comm_count(mg_hierarchy* h, long long* count);
/* all-reduces this rank entered since mg_ghost_attach (the scalars of norms / dots, the rows of the first replicated level) */
int mg_ghost_allreduce_count(mg_hierarchy* h, long long* count);

/* ---- ComplexF64 values, Int64 indices (CF64): single GPU, generic CSR ------------------------------------------------
 * The reference's solver is generic in VAL (MGparam{VAL,IND}, recursiveCycle, relax, solveMG: MGdef.jl:91-116); these entry
 * points serve VAL = ComplexF64 (frequency-domain users: shifted-Laplacian preconditioners for Helmholtz).
 *
 * Layout.  Complex arrays are interleaved (re, im) doubles - Julia ComplexF64, numpy complex128, hipDoubleComplex.  The
 *   prototypes take double*; every element count (n, n_rows, nnz, ...) counts complex numbers.
 * Applied operator.  mg_set_operator_CF64_INT64 takes the CSC arrays of the reference's AT, as the FP64 entry does, and applies
 *   AT^H - what Ac_mul_B! / mul!(target, adjoint(AT), x, alpha, beta) computes (SpMatMul.jl:9): y_i = sum_k conj(nzval_k) *
 *   x[rowval_k] over CSC column i.  The values are conjugated once, at upload.
 * Transfer operators.  P and R stay real (MGsetup.jl:80-81, SA-AMG.jl:9-10): upload them with mg_set_operator_FP64_INT64 on
 *   the CF64 handle; they are applied to complex vectors.
 * Relaxation.  relaxPrecs are complex (getRelaxPrec conjugates, MGsetup.jl:145-149); the update is x += d .* r, a pointwise
 *   complex product.
 * Norms.  ||r|| = sqrt(sum |r_i|^2), Julia's norm of a complex vector: solveMG's stopping test and resvec (which stays double).
 * Coarsest solve.  The dense inverse (column-major complex n x n) or sparse factors in the layout of
 *   mg_set_coarse_lu_FP64_INT64 / the reference's applyLUsolve_CFP64_INT64 (deps/src/parLU.cpp:69-72) with complex values,
 *   applied by the same level-scheduled triangular sweeps; or coarseSolveType "GMRES" (mg_set_coarse_gmres_CF64, below).
 * The handle.  The value type is fixed by the constructor.  Shared by both types: mg_set_cycle_type ('V', 'W', 'F'),
 *   mg_set_relax_type (0), mg_set_option, mg_set_nrhs (1), mg_finalize, mg_destroy, mg_graph_launches, mg_set_grid_hint (a
 *   no-op hint here), mg_profile_enable / _reset / _get (nothing is recorded), mg_last_error.  Every other FP64 entry point
 *   called with a CF64 handle fails with MG_ERR_STATE, and every CF64 entry point called with an FP64 handle fails with
 *   MG_ERR_STATE too; nothing is changed.
 * Refused with MG_ERR_UNSUPPORTED (and a mg_last_error message): cycle 'K' and relaxType 1 (Jac-GMRES) through the shared setters
 *   mg_set_cycle_type / mg_set_relax_type (a CF64 handle takes them through mg_set_schedule_CF64, below), the real GMRES coarse solve
 *   (mg_set_coarse_gmres_FP64: a complex handle takes mg_set_coarse_gmres_CF64), nrhs > 1 (mg_create_CF64, mg_set_nrhs, the cycle / solve / spmv entries: a complex handle's own
 *   nrhs stays 1, and blocks of right-hand sides go through the mg_block_*_CF64 / _CFP64 entry points at the end of this header, which
 *   take nrhs with each call), the _FP64 Krylov drivers
 *   (mg_pcg*, mg_bicgstab*, mg_fgmres*, mg_block_*_FP64; BiCGSTAB and FGMRES have _CFP64 forms below), mg_rap_FP64 (mg_rap_CF64 serves them), mg_transpose_hierarchy (a complex handle is flipped by
 *   mg_adjoint_hierarchy_CF64 / _CF32, below), mg_kcycle_step_async_dev_FP64, every
 *   mg_ghost_* call and mg_dist_set_tail_INT64 with a CF64 tail (the mg_dist_* handles are FP64 by construction).
 * Formats.  Generic CSR only, one streaming kernel (int32 row pointers; 64-bit beyond 2^31 - 4096 non-zeros or with the option
 *   "force_rowptr64"); the row-class, band, tile, march and small-level formats are real-valued and not used.  No HIP graphs. */
int mg_create_CF64(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out);
/* MG_OP_A only (complex nzval of AT, 2*nnz doubles); P and R go through mg_set_operator_FP64_INT64. */
int mg_set_operator_CF64_INT64(mg_hierarchy* h, long long level, long long which, long long n_rows, long long n_cols,
                               const long long* colptr, const long long* rowval, const double* nzval);
/* relaxPrecs[level]: n complex values. */
int mg_set_relax_CF64(mg_hierarchy* h, long long level, const double* d, long long n, long long relaxPre,
                      long long relaxPost);
int mg_set_coarse_dense_inverse_CF64(mg_hierarchy* h, long long n, const double* Ainv_colmajor);
/* Factors of at least lu_multi_min_rows rows (the option of the real hierarchy) run chip-wide, as mg_lu_*_CFP64 applies them,
 * on the hierarchy's stream; smaller ones in one workgroup (mg_coarse_form tells which). */
int mg_set_coarse_lu_CF64_INT64(mg_hierarchy* h, long long n, const long long* Lptr, const long long* Lcol,
                                const double* Lval, const long long* Uptr, const long long* Ucol,
                                const double* Uval, const long long* p, const long long* q);
/* x <- recursiveCycle(param,b,x,1); b, x: n complex values; nrhs must be 1; x_is_zero as for mg_cycle_FP64. */
int mg_cycle_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long x_is_zero);
/* solveMG; resvec (double, length maxIter+1, may be NULL) receives ||r0|| and ||r|| after every cycle. */
int mg_solve_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                  long long maxIter, long long* iters, double* resvec);
/* target = beta*target + alpha*Op*x on one level; alpha and beta are complex, each a (re, im) pair. */
int mg_spmv_CF64(mg_hierarchy* h, long long level, long long which, const double* alpha, const double* x,
                 const double* beta, double* y, long long nrhs);

/* ---- replaceMatrixInHierarchy on a CF64 handle (MGsetup.jl:226-270) ---------------------------------------------------------
 * A matrix whose values change and whose pattern does not (one call per outer iteration of an inversion: new medium, same
 * shifted Laplacian pattern, same P and R) is re-set-up in HBM; nothing is uploaded again and nothing re-blocked.  Value arrays
 * are in the convention of mg_set_operator_CF64_INT64: interleaved (re, im) doubles of the reference's AT (conjugated by the
 * library on the way in and back on the way out) for A, real doubles for P and R; nnz counts values and must be the stored
 * pattern's (MG_ERR_INVALID otherwise).  Common refusals: a null handle or array MG_ERR_INVALID, an FP64 handle MG_ERR_STATE.
 *
 * mg_rap_CF64 is mg_rap_FP64 for complex values: it writes the new fine values, then per level recomputes relaxPrecs[l]
 * (relaxKind 0: Jac, d = omega/a_ii, contraction off: s = fl(fl(x x) + fl(y y)), d = (fl(omega x)/s, fl(-omega y)/s); 1: SPAI, d = omega*conj(a_ii)/s_i with s_i the sum of re^2 + im^2 over COLUMN i in ascending
 * row order; omega[l] real, one per level) and As[l+1] = Rs[l]*(As[l]*Ps[l]) on its fixed pattern (csrc/mg_complex.hpp,
 * cx_rap_numeric: deterministic, no atomics; rows of any length, at most the option rap_chunk target columns at a time; the
 * option rap_groups sets how many rows of A a wavefront walks side by side, 1 being the order of mg_rap_FP64's kernel).  The
 * coarsest factorisation stays with the host, as for FP64: mg_get_values_CF64 of the coarsest level, factor, hand the solve
 * back (mg_set_coarse_dense_inverse_CF64 / mg_set_coarse_lu_CF64_INT64), mg_finalize - except with the GMRES coarsest solve, whose
 * vector d is recomputed here from omega[nlevels - 1] (see mg_set_coarse_gmres_CF64), and with the option "coarse_device_inverse" and a
 * dense inverse installed, which is rebuilt here in HBM (mg_build_coarse_dense_inverse_CF64): nothing is left to the host.  Also refused: a handle that is not
 * finalized (MG_ERR_STATE), relaxKind other than 0 or 1 (MG_ERR_INVALID), any operator with 64-bit row pointers
 * (MG_ERR_UNSUPPORTED).  These checks of arguments and state precede the first write: after such a refusal the handle cycles
 * with its old values.  (A HIP error in the middle of the re-setup, MG_ERR_HIP, may leave some levels refreshed, as for FP64.)
 * mg_rap_level_ms_CF64: device time of the last mg_rap_CF64 per level (relaxPrecs[l] and As[l+1]), out[0 .. nlevels-1), ms;
 * n must be nlevels - 1 (MG_ERR_INVALID), and a mg_rap_CF64 must have completed on the handle (MG_ERR_STATE).
 * mg_get_values_CF64 / mg_replace_values_CF64: one operator's values in stored CSR order (A: nnz complex; P, R: nnz real).
 * mg_get_relax_CF64: relaxPrecs[level], n complex values, as mg_set_relax_CF64 takes them.
 * A coarse operator As[l+1] with a row whose stored columns descend anywhere is refused (MG_ERR_UNSUPPORTED, found at upload,
 * before the first write: the kernel finds its target columns by binary search).
 * Assumed, as by mg_rap_FP64, and not validated at upload for hand-built hierarchies: the rows of every As[l+1] hold
 * no column twice and contain every column the product reaches; no row of P holds a column twice.
 * Determinism is per configuration: the order of the sums depends on the number of lane groups, which follows rap_groups and is
 * halved while the accumulator copies of a level's longest row exceed 32 KB of LDS - the same handle gives the same bits on
 * every run; handles with other options or other row lengths may differ in the last bits.
 *
 * The _CF32 forms (mg_rap_CF32, mg_rap_level_ms_CF32, mg_get_values_CF32, mg_get_relax_CF32, mg_replace_values_CF32) are the same
 * five for a CF32 handle (mg_create_CF32), with the conventions of mg_set_operator_CF32_INT64 / mg_set_relax_CF32: (re, im) float
 * pairs for A and relaxPrecs, floats for P and R; omega stays double.  The kernels are the same templates (csrc/mg_complex.hpp): a
 * single value is widened as it is loaded, every product and sum is the ComplexF64 one of mg_rap_CF64 - the same walk, lane
 * groups, LDS accumulator and order - and As[l+1] and relaxPrecs[l] are rounded to single once, where they are stored: each part
 * of each entry of As[l+1] is the correctly rounded double sum of the widened operators to within that sum's own rounding.
 * mg_rap_CF32 refuses what mg_rap_CF64 refuses, with the same codes, before the first write; a CF64 or FP64 handle is
 * MG_ERR_STATE in all five, and the _CF64 forms keep refusing a CF32 handle (MG_ERR_UNSUPPORTED).  Behind its last product and
 * inside its one synchronisation mg_rap_CF32 also refreshes what a CF32 handle derives from its operators: the coarsest operator
 * widened for the GMRES coarsest solve, then that solve's Jacobi vector from it; the explicit inverse with the option
 * "coarse_device_inverse" (singular: MG_ERR_INVALID, the previous inverse stays); on a Vanka handle with the option
 * "vanka_device_setup" every level's blocks (mg_build_vanka_CF32's kernel; a singular cell: no level's blocks are exchanged); and
 * As[1] widened for the Krylov drivers is dropped, so that the next driver call widens the new values (a Krylov operator set by
 * the caller is the caller's to refresh: mg_replace_krylov_values_CFP64).  mg_replace_values_CF32 of As[1] drops that copy too, and
 * of the coarsest operator refreshes the GMRES coarsest solve's widened copy (its Jacobi vector stays the caller's).
 * These return mg_status (below): MG_OK or an MG_ERR_* code, as every entry point of this header does. */
typedef int mg_status;   /* the status every entry point returns (MG_OK, MG_ERR_*); the older prototypes spell it int */
mg_status mg_rap_CF64(mg_hierarchy* h, const double* fine_nzval, long long nnz, long long relaxKind, const double* omega,
                      long long* levels_done);
mg_status mg_rap_level_ms_CF64(mg_hierarchy* h, double* out, long long n);
mg_status mg_get_values_CF64(mg_hierarchy* h, long long level, long long which, double* out, long long nnz);
mg_status mg_get_relax_CF64(mg_hierarchy* h, long long level, double* out, long long n);
mg_status mg_replace_values_CF64(mg_hierarchy* h, long long level, long long which, const double* nzval, long long nnz);
/* mg_rap_CF32 refuses a coarse operator As[l+1] with a row whose stored columns descend anywhere (MG_ERR_UNSUPPORTED, found at upload,
 * before anything is written), as mg_rap_FP64 and mg_rap_CF64 do. */
mg_status mg_rap_CF32(mg_hierarchy* h, const float* fine_nzval, long long nnz, long long relaxKind, const double* omega,
                      long long* levels_done);
mg_status mg_rap_level_ms_CF32(mg_hierarchy* h, double* out, long long n);
mg_status mg_get_values_CF32(mg_hierarchy* h, long long level, long long which, float* out, long long nnz);
mg_status mg_get_relax_CF32(mg_hierarchy* h, long long level, float* out, long long n);
mg_status mg_replace_values_CF32(mg_hierarchy* h, long long level, long long which, const float* nzval, long long nnz);

/* ---- the explicit inverse of the coarsest operator built on the device (csrc/mg_dense_inv.hpp) ---------------------------------------------------------------
 * A dense inverse with partial pivoting in HBM: blocked in-place Gauss-Jordan with row interchanges, panels of 64 columns, the
 * trailing update an LDS-tiled FP64 GEMM.  Pivot of a column: the largest |re| + |im| (|a| for real values) among the eligible
 * rows, ties to the lowest row, found by a two-stage reduction in a fixed order.  No atomics: a rerun gives the same bits.  Every
 * stage is a launch of its own on one stream; the pivots and the singular flag stay in device memory and the host synchronises
 * ONCE per inverse, when it reads the flag.  A zero or non-finite pivot: MG_ERR_INVALID, naming the column.
 *
 * mg_dense_inverse_FP64 / _CF64: stand-alone, on device `device`.  A: n x n column-major on the host (CF64: interleaved (re, im));
 *   out receives inv(A) in the same layout (out may be A).  Checked ahead of the first device call: a null pointer or n < 1
 *   MG_ERR_INVALID, n > 8192 MG_ERR_UNSUPPORTED.
 * mg_build_coarse_dense_inverse_FP64 / _CF64: inv(As[nlevels]) from the coarsest operator resident on the handle, installed as
 *   the coarsest solve - the state mg_set_coarse_dense_inverse_* leaves (a borrowed Schwarz handle detached, sparse factors
 *   dropped, mg_finalize due).  The _CF64 form also takes CF32 handles, whose coarsest operator is widened to ComplexF64.  The
 *   result is built into a spare buffer and exchanged with the installed inverse only when no pivot was flagged: a singular
 *   operator (MG_ERR_INVALID) leaves the previous coarsest solve in place.  Refused ahead of the first write: a null handle
 *   MG_ERR_INVALID, a handle of the other value type MG_ERR_STATE, a coarsest operator that was not uploaded MG_ERR_STATE, one
 *   with 64-bit row pointers, a sharded handle, or more rows than the option "coarse_device_inverse_max" (default and at most
 *   8192) MG_ERR_UNSUPPORTED.
 * mg_get_coarse_dense_inverse_FP64 / _CF64: the installed inverse, column-major n x n, whoever installed it; MG_ERR_STATE when
 *   the coarsest solve is not a dense inverse, MG_ERR_INVALID when n is not its order.
 * With the option "coarse_device_inverse" set on the handle, mg_rap_FP64 / mg_rap_CF64 rebuild the inverse behind their last
 *   Galerkin product, on the same stream and inside their one synchronisation, while the coarsest solve is a dense inverse:
 *   nothing of the coarsest solve is left to the host, and no mg_finalize is due.  A singular new operator is their
 *   MG_ERR_INVALID: the operators then hold the new values and the coarsest solve the previous inverse.
 *   mg_coarse_form keeps reporting kind 0. */
mg_status mg_dense_inverse_FP64(long long device, long long n, const double* A, double* out);
mg_status mg_dense_inverse_CF64(long long device, long long n, const double* A, double* out);
mg_status mg_build_coarse_dense_inverse_FP64(mg_hierarchy* h);
mg_status mg_build_coarse_dense_inverse_CF64(mg_hierarchy* h);
mg_status mg_get_coarse_dense_inverse_FP64(mg_hierarchy* h, long long n, double* out);
mg_status mg_get_coarse_dense_inverse_CF64(mg_hierarchy* h, long long n, double* out);

/* ---- adjointHierarchy on a complex handle (transposeHierarchy for complex VAL, MGsetup.jl:274-318) ----------------------------
 * The flip between the forward system A x = b and the adjoint system A' x = b (A' = conj(A)^T, Julia's `'`) that an inversion
 * makes in every outer iteration, on the resident hierarchy: As[l] <- As[l]' on every level, relaxPrecs[l] <- conj(relaxPrecs[l]),
 * Ps[l] <- Rs[l]' (Rs[l] keeps its values: the reference's second assignment reads the new Ps[l]), and the coarsest solve for the
 * adjoint operator: the dense inverse replaced by its conjugate transpose in place ((A')^-1 = (A^-1)'; ComplexF64 on CF32 handles
 * too), the GMRES coarsest solve's vector d conjugated (MGsetup.jl:304-305).  mg_adjoint_hierarchy_CF64 serves CF64 handles (V / W /
 * F / K cycles, Jac / SPAI / Jac-GMRES relaxation), mg_adjoint_hierarchy_CF32 CF32 handles (V / W / F, Jac / SPAI); hierarchies of
 * one level included.  mg_transpose_hierarchy keeps refusing complex handles.
 * Values and column indices never leave HBM (csrc/mg_complex.hpp, cx_adj_*): per operator the entries of every column are counted
 * (integer atomics), the n_cols counts are read back (4 bytes per column), scanned on the host into the new row pointers and cut
 * into row blocks by the upload's rule (pointers and block table go back), every entry's row index is scattered into its column's
 * segment, and every entry is then written - conjugated; the real values of R copied - to its place in the segment: the number
 * of entries of that column with a smaller row index.  The result is the stored-order CSR of the adjoint, bit for bit what a host
 * conjugate transpose with sorted indices gives, the same bits on every run; no floating-point atomics.  The transposed pattern
 * cached for SPAI re-setups is dropped (the next mg_rap_CF64 rebuilds it), a CF32 handle's widened coarsest operator is rebuilt
 * from the new As[end] and its widened Krylov operator from the new As[1] (at the next driver call); a Krylov operator the caller
 * set (mg_set_krylov_operator_CFP64_INT64) is the caller's to flip and is left alone.  The call ends with the finalization path.
 * Refused, every check before the first write, so that the handle cycles with its old bits afterwards: a null handle
 * MG_ERR_INVALID; a handle that is not finalized, an FP64 handle, the _CF64 entry on a CF32 handle or the reverse MG_ERR_STATE;
 * any operator with 64-bit row pointers, a column of more than 4096 entries in any A or R (the ranking reads a column once per
 * entry of it), a coarsest solve held as sparse factors (single-workgroup or chip-wide) or a Schwarz coarsest solve
 * MG_ERR_UNSUPPORTED - hand the adjoint hierarchy over with the set_* calls then.  A HIP error in the middle (MG_ERR_HIP) leaves a
 * partly flipped handle that is NOT finalized: every entry point refuses it until it has been uploaded again, as for
 * mg_transpose_hierarchy. */
mg_status mg_adjoint_hierarchy_CF64(mg_hierarchy* h);
mg_status mg_adjoint_hierarchy_CF32(mg_hierarchy* h);

/* ComplexF32 factors on a CF32 handle (a parallelJuliaSolver(ComplexF32, Int64) as param.LU): Lval, Uval interleaved floats.  The
 * coarsest solve applies them to the cycle's own single bc - no widening and narrowing passes around it - with the arithmetic of
 * mg_lu_*_CFP32, in one workgroup below lu_multi_min_rows rows and chip-wide from there on, for a vector and for blocks.  A CF64
 * or FP64 handle refuses it (MG_ERR_STATE); mg_set_coarse_lu_CF64_INT64 on a CF32 handle keeps the widened ComplexF64 route. */
mg_status mg_set_coarse_lu_CF32_INT64(mg_hierarchy* h, long long n, const long long* Lptr, const long long* Lcol,
                                      const float* Lval, const long long* Uptr, const long long* Ucol,
                                      const float* Uval, const long long* p, const long long* q);

/* ---- Float32 / ComplexF32 Schwarz sweeps --------------------------------------------------------------------------------------
 * The multiplicative Schwarz preconditioner (mg_dd_*, above) with VAL = Float32 / ComplexF32: DomainDecompositionParam{VAL,IND} is
 * generic in VAL, computeResidualAtIdx and solveSubDomain run in VAL (DDSerial.jl:4-20, 183-187) and parallelJuliaSolver has the three
 * single forms.  A handle records its value type with the factor applier's codes - 0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32
 * (mg_dd_info[0]) - and keeps the operator, the caller's factors, the packed arenas and the work vectors in float: half the HBM of a
 * double handle, no double copy beside it.
 * create: valA in float (interleaved (re, im) for CFP32), the CSR indices Int64 - the reference's AT is Int64-indexed whatever VAL is.
 * set_factor: the three forms parLU has - (Float32, UInt32), (ComplexF32, UInt32), (ComplexF32, Int64): column indices and
 * permutations in the index type of the name, row pointers Int64; there is no (Float32, Int64) form.  apply / dd0_apply: b and x in
 * float, host pointers or HBM (_dev); mg_dd_finalize, mg_dd_info, mg_dd_time_dev (b_dev / x_dev then point to float data) and
 * mg_dd_destroy serve every kind.  doTranspose: the transposed (CFP32: conjugate-transposed) single factors - moving a value or
 * flipping a sign bit is exact.  A member of at least lu_multi_min_rows rows gets a single applier of its own (mg_lu_*_FP32 /
 * _CFP32) and its colour runs in sequence, as for double handles.
 * Arithmetic: the single factor applier's contract.  Values, factors, b, x, r and y are STORED in single; every residual row and every
 * triangular row is EVALUATED in double - operands widened before each product, the sum in the order of the double kernels, one
 * rounding to single on the store; x[I] += t is one single add.  A deliberate deviation from the reference, which sums in VAL.
 * Every mg_dd_* entry point called on a handle of another kind fails with MG_ERR_STATE, names the entry points that serve the handle
 * and leaves it usable.
 * mg_set_coarse_dd accepts a ComplexF32 handle on a CF32 hierarchy (mg_create_CF32): the sweep runs from zero on the cycle's own
 * complex64 coarsest vectors - no widened pair is allocated; mg_coarse_form reports 4.  Every other pairing of kinds is MG_ERR_STATE
 * with both named; a ComplexF64 handle on a CF32 hierarchy stays MG_ERR_UNSUPPORTED.  Unchanged refusals for such a hierarchy: blocks
 * (nrhs > 1), sharded forms, mg_adjoint_hierarchy_CF32, HIP graphs of its sub-cycles. */
mg_status mg_dd_create_FP32_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA,
                                  const float* valA, long long numSub, const long long* idxptr, const unsigned int* idx,
                                  const long long* color, mg_dd** out);
mg_status mg_dd_create_CFP32_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA,
                                   const float* valA, long long numSub, const long long* idxptr, const unsigned int* idx,
                                   const long long* color, mg_dd** out);
mg_status mg_dd_set_factor_FP32_UINT32(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const unsigned int* Lcol,
                                       const float* Lval, const long long* Uptr, const unsigned int* Ucol, const float* Uval,
                                       const unsigned int* p, const unsigned int* q);
mg_status mg_dd_set_factor_CFP32_UINT32(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const unsigned int* Lcol,
                                        const float* Lval, const long long* Uptr, const unsigned int* Ucol, const float* Uval,
                                        const unsigned int* p, const unsigned int* q);
mg_status mg_dd_set_factor_CFP32_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol,
                                       const float* Lval, const long long* Uptr, const long long* Ucol, const float* Uval,
                                       const long long* p, const long long* q);
mg_status mg_dd_apply_FP32(mg_dd* dd, const float* b, float* x, long long n, long long niter, long long doTranspose);
mg_status mg_dd_apply_dev_FP32(mg_dd* dd, const float* b_dev, float* x_dev, long long n, long long niter, long long doTranspose);
mg_status mg_dd_apply_CFP32(mg_dd* dd, const float* b, float* x, long long n, long long niter, long long doTranspose);
mg_status mg_dd_apply_dev_CFP32(mg_dd* dd, const float* b_dev, float* x_dev, long long n, long long niter, long long doTranspose);
mg_status mg_dd0_apply_FP32(mg_dd* dd, const float* b, float* x, long long n, long long doTranspose);
mg_status mg_dd0_apply_dev_FP32(mg_dd* dd, const float* b_dev, float* x_dev, long long n, long long doTranspose);
mg_status mg_dd0_apply_CFP32(mg_dd* dd, const float* b, float* x, long long n, long long doTranspose);
mg_status mg_dd0_apply_dev_CFP32(mg_dd* dd, const float* b_dev, float* x_dev, long long n, long long doTranspose);

/* ---- The GMRES coarsest solve on a complex handle ----------------------------------------------------------------------------
 * coarseSolveType "GMRES" for complex handles (MGsetup.jl:335-336, MGcycle.jl:152-164): d = param.LU = relaxParam ./ diag(A_c), n
 * complex128 values for CF64 AND CF32 handles (as the other complex coarse setters); the coarsest solve is x .= 0 and ONE restart of
 * KrylovMethods.fgmres(A_c, b, 10, tol = 0.01, maxIter = 1) preconditioned by v -> d .* v, in the reference's operation order
 * (modified Gram-Schmidt, h_k = dot(v_k, w) conjugating v_k, w -= h_k v_k, k ascending).  No factorisation, nothing to redo on the
 * host when the matrix changes.  The setter replaces whatever coarsest solve was set and detaches a borrowed Schwarz handle; an FP64
 * handle: MG_ERR_STATE; n other than the coarsest order: mg_finalize fails with MG_ERR_INVALID.  mg_finalize allocates the work set
 * (11 basis vectors, 10 preconditioned vectors, a table of 121 scalars with a pinned readback); no cycle allocates.
 * The solve is enqueued speculatively and whole: all 10 Arnoldi steps, ONE readback of the table (||b||^2 and, per step, h_0 .. h_i
 * and ||w||^2), ONE host synchronisation; the host replays the columns, breaks at the first err / ||b|| <= 0.01, and x = Z[:, :used] y
 * is one more launch.  Steps behind the break are computed and not read.  b = 0: x = 0.  EVERY COARSEST SOLVE THEREFORE ADDS ONE HOST
 * SYNCHRONISATION TO THE CYCLE: one per V-cycle, 2^(levels - 2) per W- or K-cycle - also for mg_cycle_dev_CFP64, which otherwise
 * returns without one, and per preconditioner application of the _CFP64 drivers.  Launches: a step is the product w = A_c z_i (which also
 * leaves the partials of dot(v_0, w)) and either a chain of i + 1 Gram-Schmidt passes and one normalising pass (i + 3 launches; every
 * pass sums the partials of the pass before it, no final-sum launch in between) or, on coarsest levels of at most 8192 rows, ONE
 * one-workgroup launch that holds w in registers (2 launches per step).  The option coarse_gmres_tail_rows (read at every solve) moves
 * that threshold: -1 the default, 0 the chain everywhere.  mg_coarse_form reports kind 3 and the launch count of the path in use (78
 * for the chain, 22 for the one-workgroup form).  Sums are deterministic (no atomics): a rerun gives the same bits.
 * Served: V / W / F / K cycles with Jac / SPAI / Jac-GMRES smoothing on CF64 handles, V / W / F with Jac / SPAI on CF32 handles, a
 * hierarchy of one level (the solve alone), mg_solve_*, the _CFP64 drivers, mg_rap_CF64 (it recomputes d = omega[nlevels - 1] / diag(A_c)
 * on the device after the last Galerkin product: omega then holds nlevels entries, and the host has nothing to factor).
 * A CF32 handle runs this solve in ComplexF64 like its other coarsest solves: bc widened, the solve on a ComplexF64 copy of the
 * coarsest operator kept for it, xc narrowed.  The reference would run this fgmres in ComplexF32: a deliberate deviation of the order
 * of the single unit roundoff (more accurate).
 * Refused with MG_ERR_UNSUPPORTED unless the handle's option coarse_gmres_blocks is set (below): every mg_block_*_CF64 / _CFP64 entry
 * point with nrhs > 1.
 * mg_coarse_gmres_CF64: the coarsest solve alone on host vectors of n = coarsest order complex values; steps (the columns used), flag
 * (0: the estimate met 0.01; -1: it did not within 10 steps; -9: b = 0) and resvec10 (err_i / ||b|| of the steps used; room for 10) may
 * be NULL.  MG_ERR_STATE on a handle that is not finalized or whose coarsest solve is not GMRES; MG_ERR_INVALID for another n. */
mg_status mg_set_coarse_gmres_CF64(mg_hierarchy* h, long long n, const double* d);
mg_status mg_coarse_gmres_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long* steps, long long* flag,
                               double* resvec10);

/* ---- the block GMRES coarsest solve (MGcycle.jl:165-167): blocks of right-hand sides on a GMRES-coarse complex handle -------------
 * OPT-IN: mg_set_option(h, "coarse_gmres_blocks", 1) (default 0; read at every call).  With 0 a block of nrhs > 1 on a complex handle
 * whose coarsest solve is GMRES is refused with MG_ERR_UNSUPPORTED, word for word as before this solve existed.  With 1 these entry
 * points serve such a handle for 1 <= nrhs <= 16: mg_block_cycle_CF64, mg_block_solve_CF64, mg_block_spmv_CF64,
 * mg_block_cycle_dev_CFP64, mg_block_bicgstab[_dev]_CFP64, mg_block_fgmres[_dev]_CFP64 (CF64 and CF32 handles as each of them serves
 * them; a CF32 handle runs the solve in ComplexF64 on the widened coarsest operator).
 * The coarsest solve of a block is X .= 0 and ONE restart of blockFGMRES(A_c, B, 10, tol = 0.01, maxIter = 1, M = V -> d .* V) with the
 * same Jacobi vector d as the single-vector solve: V_0, xi_0 = cholqr2(B); per step Z_j = d.*V_j, W = A_c Z_j, block modified
 * Gram-Schmidt in ascending order (H_ij = V_i^H W, W -= V_i H_ij), V_{j+1}, H_{j+1,j} = cholqr2(W) - Cholesky QR applied twice with the
 * semidefinite factor (real pivots; a column with g <= 0 or d <= 1e-14 g is dropped: a zero row of R, a zero column of Q).  THE COLUMNS
 * OF A BLOCK ARE COUPLED: the result is not that of nrhs single-vector solves, and the stopping test is on the whole block,
 * ||xi - H Y||_F / ||B||_F <= 0.01.
 * The restart is enqueued whole - front 3 launches, step j: j + 5 (the product, V_0^H W, j + 1 Gram-Schmidt passes, two Cholesky
 * passes; every pass sums the k x k partials of the pass before it and does the small algebra itself, no launch only sums) - then ONE
 * copy of the table (||B||_F^2, xi_0, every H_ij: 270 KB at nrhs = 16) and ONE HOST SYNCHRONISATION PER COARSEST SOLVE, as for the
 * single-vector form; the host replays the block least squares, breaks at the first estimate <= 0.01, and X = sum_j Z_j Y_j is one
 * copy and one more launch: 99 launches in all (mg_block_coarse_form).  No atomics: a rerun gives the same bits.  B = 0: X = 0.
 * The work set (11 + 10 blocks of n_c x nrhs, partials, table) belongs to the block work set: allocated at the first block call,
 * grown when a larger nrhs arrives, never inside a cycle.  nrhs = 1 through the block entry points is the single-vector solve.
 * Still refused (MG_ERR_UNSUPPORTED): blocks on K-cycle / Jac-GMRES hierarchies, with a Schwarz coarsest solve, nrhs > 16, the
 * sharded forms and FP64 handles (the real GMRES coarsest solve is column by column there already).
 * mg_block_coarse_gmres_CF64: the block solve alone on host blocks, column-major n x nrhs (n = the coarsest order) like the other host
 * block entry points; steps, flag (0 / -1 / -9) and resvec10 (the estimates of the steps used) of the whole block may be NULL.
 * MG_ERR_STATE on a handle that is not finalized or whose coarsest solve is not GMRES; MG_ERR_UNSUPPORTED for nrhs > 1 without the
 * option; MG_ERR_INVALID for another n.
 * Blocks of few values (n_c * nrhs <= 1024 by default) take a one-workgroup form of everything behind the product instead of the
 * chain: the same passes one after the other in ONE launch, 1 launch for the front and 2 per step, 22 in all.  The option
 * coarse_gmres_tail_rows moves that threshold too (compared with n_c * nrhs for a block; 0: the chain everywhere; at most 8192).
 * mg_block_coarse_form: info[0] = 1 where blocks are served on this handle's GMRES coarsest solve (0 otherwise), info[1] = kernel
 * launches of one block solve of nrhs columns, info[2] = the path in use for them (0: the chain of grid-wide passes, 1: the
 * one-workgroup form). */
mg_status mg_block_coarse_gmres_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long* steps,
                                     long long* flag, double* resvec10);
mg_status mg_block_coarse_form(mg_hierarchy* h, long long nrhs, long long* info);

/* ---- Jac-GMRES smoothing and the K-cycle on a CF64 handle (MGcycle.jl:35-50,72-76,96-98; FGMRES.jl:48-126) ------------------------
 * mg_set_schedule_CF64 sets cycleType ('V', 'W', 'F' or 'K') and relaxType (0: Jac / SPAI, 1: Jac-GMRES) of a CF64 handle in one
 * call and drops `finalized` (mg_finalize allocates Z / AZ of the relaxations the schedule needs).  Other letters or types:
 * MG_ERR_INVALID; a CF32 handle: MG_ERR_UNSUPPORTED (its own form: mg_set_schedule_CF32, below); an FP64 handle: MG_ERR_STATE.  The shared setters keep refusing 'K' and type 1.
 * A relaxation is FGMRES_relaxation with the Jacobi preconditioner d: one kernel launch per direction (the product w = A z_j, the
 * next direction d.*w and the partial sums of column j of H = (AZ)'(AZ) and of xi[j] = dot(w, r0) in one walk over the rows), one
 * launch that sums all partials, ONE host synchronisation per relaxation; the host then replays the reference's loop on the leading
 * blocks of H (break at the first residual estimate below 1e-5) and x += Z t is one more launch.  The K-cycle runs its two FGMRES
 * steps with one synchronisation each.  Sums are deterministic (no atomics).  relaxPre / relaxPost above 8 with Jac-GMRES:
 * mg_finalize fails with MG_ERR_UNSUPPORTED.  On such a handle mg_cycle_CF64, mg_solve_CF64 and the _CFP64 drivers work unchanged; the
 * block entry points (mg_block_*_CF64 / _CFP64) return MG_ERR_UNSUPPORTED unless the option kcycle_blocks is set (the section on
 * blocks at the end), and mg_rap_CF64 serves every schedule (it recomputes
 * operators and relaxPrecs only).
 * mg_fgmres_relax_CF64: one such relaxation on As[level] and relaxPrecs[level] with host vectors - the reference's exported
 * FGMRES_relaxation with the diagonal preconditioner: x += Z t for the residual r0 (n complex values each; 1 <= level < nlevels,
 * 1 <= inner <= 8, a finalized CF64 handle of any schedule).  H_out (inner x inner complex, row-major), xi_out (inner complex),
 * rnorms_out (inner doubles; zero behind `used`) and used_out may be NULL; H and xi hold the summed Gram scalars of ALL inner
 * directions, also those behind a break. */
mg_status mg_set_schedule_CF64(mg_hierarchy* h, long long cycleType, long long relaxType);
mg_status mg_fgmres_relax_CF64(mg_hierarchy* h, long long level, const double* r0, double* x, long long n, long long inner,
                               double tol, double* H_out, double* xi_out, double* rnorms_out, long long* used_out);

/* ---- The same on a CF32 handle, OPT-IN: mg_set_option(h, "single_kcycle", 1) (default 0; read by mg_finalize and at every call) ------
 * The reference's configuration for Helmholtz - the K-cycle (or Jac-GMRES smoothing) on a ComplexF32 hierarchy, singlePrecision=True.
 * Without the option a CF32 handle refuses both as before: mg_set_schedule_CF32 and mg_fgmres_relax_CF32 return MG_ERR_UNSUPPORTED, and
 * so does mg_finalize behind mg_set_vanka_relax_CF32(h, 'K').  With it mg_set_schedule_CF32 takes what mg_set_schedule_CF64 takes, and
 * mg_finalize accepts 'K' and relaxation type 1 (Z / AZ of the relaxations in complex64: half the bytes; relaxPre / relaxPost above 8
 * with Jac-GMRES stay MG_ERR_UNSUPPORTED).  Served then, one right-hand side: V / W / F / K with Jac / SPAI / Jac-GMRES, K with the
 * Vanka smoothers, every coarsest solve a CF32 handle serves, through mg_cycle_CF32, mg_solve_CF32, mg_cycle_dev_CFP64 and the mixed
 * closure of mg_bicgstab[_dev]_CFP64 / mg_fgmres[_dev]_CFP64; the synchronisations per cycle are those of a CF64 handle.  Still
 * MG_ERR_UNSUPPORTED: every block entry point on such a schedule (unless the option kcycle_blocks is set as well), a Schwarz coarsest solve, 'K' / type 1 through the shared setters
 * mg_set_cycle_type / mg_set_relax_type.
 * ARITHMETIC.  Z and AZ are complex64; w = A z_j, its products and row sums, and the next direction d.*w are formed in single, in
 * stored order (the arithmetic of the CF32 sweep and residual kernels).  DEVIATION from the reference, which forms H, xi and the small
 * least squares in ComplexF32: here the Gram scalars are formed in DOUBLE - w, r0 and AZ_i are widened before they are multiplied, so
 * every product of two singles is exact and only the fixed-order sums round - and the least squares, the residual estimates and the
 * break at 1e-5 are the ComplexF64 host algebra.  (In single the estimate cancels down to about sqrt(2^-24) ||r0||: the break would be
 * noise.)  x += Z t: t in double, the sum of an element formed in double in direction order, rounded once on the store.
 * mg_fgmres_relax_CF32: as mg_fgmres_relax_CF64 with complex64 r0 and x (n (re, im) float pairs each); H_out, xi_out, rnorms_out stay
 * double.  Z_out / AZ_out (may be NULL) receive the n x inner column-major complex64 Z and AZ of the relaxation (all inner
 * directions).  A CF64 or FP64 handle: MG_ERR_STATE. */
mg_status mg_set_schedule_CF32(mg_hierarchy* h, long long cycleType, long long relaxType);
mg_status mg_fgmres_relax_CF32(mg_hierarchy* h, long long level, const float* r0, float* x, long long n, long long inner, double tol,
                               double* H_out, double* xi_out, double* rnorms_out, long long* used_out, float* Z_out, float* AZ_out);

/* ---- The Vanka cell-block smoother in the complex cycle (relaxation type 2; MGcycle.jl:46-52,99-100, Vanka.jl:372-434) -------------
 * mg_set_vanka_CF64 / mg_set_vanka_CF32 bind the cells' blocks of one level of a CF64 / CF32 handle, as mg_set_vanka_FP64 does for a
 * real level and with its checks: As[level] uploaded first (MG_ERR_STATE), no 64-bit row pointers (MG_ERR_UNSUPPORTED), (dim, n,
 * includePressure) against the operator's rows (MG_ERR_INVALID), VankaType FULL_VANKA_RB (1), ECON_VANKA_RB (3) or FULL_VANKA_ADD (5)
 * (others MG_ERR_UNSUPPORTED).  D_blocks: LocalBlocks of setupVankaFacesPreconditioner, (bs*bs) x prod(n) column-major ComplexF32 -
 * bs*bs*cells interleaved (re, im) float pairs, for both precisions.  A CF64 level promotes them to double; a CF32 level applies them
 * as stored, every product and sum in single.  The blocks are copied and released with the handle.  An FP64 handle, or the other
 * precision's entry: MG_ERR_STATE.
 * mg_set_vanka_relax_CF64 / _CF32 put the handle into relaxation type 2 together with its cycleType ('V', 'W', 'F', 'K'; other
 * letters MG_ERR_INVALID) and drop `finalized`.  mg_set_schedule_CF64(h, c, 2) stays MG_ERR_INVALID and mg_set_relax_type(h, 2) on a
 * complex handle MG_ERR_UNSUPPORTED; mg_set_schedule_CF64(h, c, 0 | 1) or mg_set_relax_type(h, 0) afterwards leave Vanka mode.
 * mg_finalize then asks of every non-coarsest level blocks that serve exactly its rows (none: MG_ERR_STATE; another size:
 * MG_ERR_INVALID) and the pointwise slot of mg_set_relax_CF64 / _CF32, which carries relaxPre / relaxPost and whose values nothing
 * reads; 'K' on a CF32 handle is MG_ERR_UNSUPPORTED unless its option single_kcycle is set.  The cycle runs relaxPre / relaxPost Vanka iterations of x in place from the
 * level's own CSR (a count of 0: none).  A level entered with x = 0 is zero-filled and its first pass reads b and the blocks only (no
 * matrix walk; the one pass of FULL_VANKA_ADD altogether) - bit-identical to the general pass on a zero x, which x_is_zero = 0 runs.
 * Served: mg_cycle_*, mg_solve_*, the _CFP64 drivers and their _dev forms.  MG_ERR_UNSUPPORTED: every block entry point
 * (mg_block_*), mg_rap_CF64 (it knows Jac and SPAI only: set the hierarchy up on the host and upload again), mg_adjoint_hierarchy_*.
 * BLOCKS, OPT-IN: mg_set_option(h, "vanka_blocks", 1) (default 0; read at every call).  With 1 the mg_block_* entry points serve a
 * handle in relaxation type 2 for 1 <= nrhs <= 16 and the cycles V / W / F: mg_block_cycle_CF64, mg_block_solve_CF64,
 * mg_block_spmv_CF64, mg_block_cycle_dev_CFP64, mg_block_bicgstab[_dev]_CFP64, mg_block_fgmres[_dev]_CFP64 (CF64 and CF32 handles as
 * each of them serves them today).  The smoother runs on the row-major block in place (the _blk kernels of mg_vanka.hpp); column c
 * holds the bits of the one-vector smoother on column c, the from-zero pass is decided for the whole block, and the delta buffer
 * (cells x bs x nrhs) grows with the block work set.  The K-cycle, nrhs > 16 and a Schwarz coarsest solve stay MG_ERR_UNSUPPORTED,
 * X untouched.  With 0 every return code and message is what it was before the option existed.
 * DEVICE SET-UP OF THE BLOCKS, OPT-IN.  mg_build_vanka_CF64 / _CF32 are mg_set_vanka_* with (VankaType, w, nw) in the place of
 * D_blocks: the checks are the same, the blocks are built in HBM from the level's resident operator (as mg_vanka_build_blocks_*
 * above; a CF32 level's float pairs are widened, the elimination runs in double for both precisions; nw = 2 with type 3:
 * MG_ERR_INVALID) and the level remembers (VankaType, w).  A singular cell: MG_ERR_INVALID, the level keeps what it had.
 * mg_get_vanka_blocks_CF64 / _CF32 read a level's blocks back (count = bs*bs*prod(n) ComplexF32 values; no blocks: MG_ERR_STATE).
 * mg_set_option(h, "vanka_device_setup", 1) (default 0; read at every call): mg_rap_CF64 then serves a CF64 handle in relaxation
 * type 2 - new fine values, the numeric Galerkin products, and every relaxed level's blocks built again with that level's
 * remembered (VankaType, w), each behind the product that feeds it; relaxKind and omega are validated and not used.  A level
 * whose blocks came from mg_set_vanka_CF64 has nothing remembered: MG_ERR_STATE before the first write.  A singular cell on any
 * level: MG_ERR_INVALID after the products (the operators hold the new values, every level keeps its previous blocks).  With 0
 * mg_rap_CF64 refuses a Vanka handle with the code and message it always had; CF32 handles stay MG_ERR_UNSUPPORTED there
 * (mg_rap_CF32 serves a CF32 Vanka handle under the same option, with mg_build_vanka_CF32's kernel). */
mg_status mg_build_vanka_CF64(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure,
                              long long VankaType, const double* w, long long nw);
mg_status mg_build_vanka_CF32(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure,
                              long long VankaType, const double* w, long long nw);
mg_status mg_get_vanka_blocks_CF64(mg_hierarchy* h, long long level, float* out, long long count);
mg_status mg_get_vanka_blocks_CF32(mg_hierarchy* h, long long level, float* out, long long count);
mg_status mg_set_vanka_CF64(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure,
                            long long VankaType, const float* D_blocks);
mg_status mg_set_vanka_CF32(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure,
                            long long VankaType, const float* D_blocks);
mg_status mg_set_vanka_relax_CF64(mg_hierarchy* h, long long cycleType);
mg_status mg_set_vanka_relax_CF32(mg_hierarchy* h, long long cycleType);

/* ---- ComplexF64 Krylov drivers on a CF64 handle (suffix CFP64, the reference's own) ---------------------------------------
 * solveBiCGSTAB_MG / solveGMRES_MG (SolveFuncs.jl:85-133) for VAL = ComplexF64: KrylovMethods.bicgstb / fgmres with one cycle
 * of the handle's hierarchy from x = 0 as preconditioner, every vector resident in HBM across iterations.  The way Helmholtz
 * problems are solved: the Krylov method runs on the (nearly) undamped operator - the handle's KRYLOV OPERATOR - and the
 * hierarchy is built on a damped (shifted) copy of it.
 *
 * mg_set_krylov_operator_CFP64_INT64 takes the CSC arrays of the system operator's AT, exactly as mg_set_operator_CF64_INT64
 * takes As (values conjugated once at upload, the same rule for the width of the row pointers); n must be the fine level's
 * (MG_ERR_INVALID).  colptr == NULL clears it (also on a handle that is not finalized); without one the drivers apply As[1].
 * Setting one needs a finalized handle (MG_ERR_STATE otherwise) and leaves it finalized.  mg_finalize refuses (MG_ERR_INVALID) a
 * handle whose As[1] was re-set with another order than its Krylov operator's: clear the operator, finalize, set a matching one.
 *
 * Arguments, flags and the layout of resvec of the drivers are those of mg_bicgstab_FP64 / mg_fgmres_FP64 (above); b and x hold
 * n complex values, interleaved (re, im); x goes in and out; the _dev forms take device pointers on a 16-byte boundary.  Dots
 * are Julia's, dot(a, b) = sum conj(a_i) b_i; BiCGSTAB breaks down (flag -2) on rho == 0 or omega == 0 as complex numbers; the
 * FGMRES rotations have a complex cosine and a real sine.  inner in [1,64]; the work space ((2*inner+2) complex vectors of n
 * for FGMRES, 6 for BiCGSTAB) is allocated at the first call and released with the handle.  Host synchronisations per
 * iteration: BiCGSTAB 4, FGMRES 1 per inner step.  Refused: an FP64 handle or a handle not finalized (MG_ERR_STATE); a null
 * vector, maxIter < 0, a wrong n, inner outside [1,64], a device vector off a 16-byte boundary (MG_ERR_INVALID).  Not served
 * for complex values: PCG (the operators in question are not Hermitian positive definite).  These entry points take one right-hand
 * side; a block of them goes to mg_block_bicgstab[_dev]_CFP64 / mg_block_fgmres[_dev]_CFP64 (at the end of this header). */
int mg_set_krylov_operator_CFP64_INT64(mg_hierarchy* h, long long n, const long long* colptr, const long long* rowval,
                                       const double* nzval);
/* New values (nnz complex, the AT convention) on the pattern of the Krylov operator set last: a copy and one conjugation in HBM,
 * no re-blocking.  No operator set: MG_ERR_STATE; nnz different from its pattern: MG_ERR_INVALID. */
int mg_replace_krylov_values_CFP64(mg_hierarchy* h, const double* nzval, long long nnz);
int mg_bicgstab_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol, long long maxIter,
                      long long* iters, long long* flag, double* resvec, long long* nres);
int mg_bicgstab_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, double tol, long long maxIter,
                          long long* iters, long long* flag, double* resvec, long long* nres);
int mg_fgmres_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, long long inner, double tol,
                    long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
int mg_fgmres_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long inner, double tol,
                        long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
/* One cycle on device vectors (x_is_zero: 0 or 1), enqueued on the handle's stream: no host copy, no synchronisation - except the ones
 * the schedule itself needs: one per Jac-GMRES relaxation and K-cycle step, and one per coarsest solve with the GMRES coarsest solve
 * (mg_set_coarse_gmres_CF64).  The drivers above pay the same per preconditioner application: BiCGSTAB two cycles per iteration, FGMRES
 * one per inner step. */
int mg_cycle_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long x_is_zero);
/* The fused complex vector passes of those drivers on their own (csrc/mg_cxvec.hpp): device vectors of n complex values on a
 * 16-byte boundary (MG_ERR_INVALID otherwise), asynchronous on `stream`, deterministic two-pass sums (no atomics) into out_dev
 * (device doubles).  workspace_dev: 8192 doubles.  Complex scalars are (re, im) pairs in HOST memory; xs_dev / ys_dev / vs_dev
 * are HOST arrays of device pointers, h_host holds m complex coefficients.
 *   dots: out[2c], out[2c+1] = dot(xs[c], ys[c]), c < k <= 4          scale: y = a x
 *   bicg_p: p = r + beta (p - omega v)                                bicg_s: r -= alpha v, out[0] = ||r||^2
 *   bicg_ts: out = (re, im of dot(t, s), dot(t, t))
 *   bicg_xr: x += alpha phat + omega shat, r -= omega t, out = (||r||^2, re, im of dot(rtld, r))
 *   gs_update: w -= sum_{j<m} h[j] vs[j] one after the other (m <= 64, 8 per pass), out (optional) = ||w||^2 */
int mg_cvec_dots_dev_CFP64(long long k, const double* const* xs_dev, const double* const* ys_dev, long long n,
                           double* workspace_dev, double* out_dev, void* stream);
int mg_cvec_scale_dev_CFP64(const double* a, const double* x, double* y, long long n, void* stream);
int mg_cvec_bicg_p_dev_CFP64(const double* beta, const double* omega, const double* r, const double* v, double* p,
                             long long n, void* stream);
int mg_cvec_bicg_s_dev_CFP64(const double* alpha, const double* v, double* r, long long n, double* workspace_dev,
                             double* out_dev, void* stream);
int mg_cvec_bicg_ts_dev_CFP64(const double* t, const double* s, long long n, double* workspace_dev, double* out_dev,
                              void* stream);
int mg_cvec_bicg_xr_dev_CFP64(const double* alpha, const double* omega, const double* phat, const double* shat,
                              const double* t, const double* rtld, double* x, double* r, long long n,
                              double* workspace_dev, double* out_dev, void* stream);
int mg_cvec_gs_update_dev_CFP64(long long m, const double* h_host, const double* const* vs_dev, double* w, long long n,
                                double* workspace_dev, double* out_dev, void* stream);
/* The one-pass Gram kernel of mg_block_fgmres_CFP64 on its own: out_dev (k x k complex, row-major) = X^H Y for two row-major device
 * blocks [n][k] on a 16-byte boundary, 1 <= k <= 16 (k < 1, n < 1: MG_ERR_INVALID; k > 16: MG_ERR_UNSUPPORTED); x_dev == y_dev is
 * served and reads the block once.  Asynchronous on `stream`; a deterministic two-stage sum.  workspace_dev: 2048 * k * k doubles. */
int mg_cblk_gram_dev_CFP64(const double* x_dev, const double* y_dev, long long n, long long k, double* workspace_dev,
                           double* out_dev, void* stream);

/* ---- ComplexF32 hierarchies (CF32): the single-precision cycle inside the ComplexF64 Krylov drivers ------------------------
 * The reference's VAL = ComplexF32 (getMGparam: singlePrecision, MGdef.jl:151; MGsetup.jl:31-33, 79-82, 108-110): As and relaxPrecs
 * are ComplexF32, Ps / Rs Float32, every level vector ComplexF32; products and row sums are formed in single precision in stored
 * order by the same kernels, the same row blocks and the same cycle code as a CF64 handle's (csrc/mg_complex.hpp).  Per non-zero
 * the stream kernel moves 12 B for A (8 value + 4 index) against 20, 8 B for P / R against 12, and 8 B per vector element against
 * 16.  ||r||^2 of mg_solve_CF32 is summed in double.
 *
 * mg_create_CF32 makes the handle.  mg_set_operator_CF32_INT64 takes the reference's AT arrays as the CF64 entry does: for MG_OP_A
 * nzval holds nnz interleaved (re, im) float pairs (conjugated here once), for MG_OP_P / MG_OP_R nnz floats.  mg_set_relax_CF32
 * takes n (re, im) float pairs.  mg_cycle_CF32 / mg_solve_CF32 / mg_spmv_CF32 take host vectors of (re, im) float pairs; alpha and
 * beta are (re, im) float pairs; resvec is double.
 *
 * The coarsest solve stays ComplexF64, as Julia's lu of a ComplexF32 matrix does (UMFPACK has no single form; MGsetup.jl:350,
 * MGcycle.jl:177-178): set it with mg_set_coarse_dense_inverse_CF64 / mg_set_coarse_lu_CF64_INT64 (double factors); the cycle
 * widens bc, runs the CF64 coarsest kernels and narrows xc.
 *
 * The mixed branch of getMultigridPreconditioner (SolveFuncs.jl:52-58) is served by the ComplexF64 Krylov entry points above, which
 * accept a CF32 handle: mg_set_krylov_operator_CFP64_INT64, mg_replace_krylov_values_CFP64, mg_bicgstab[_dev]_CFP64,
 * mg_fgmres[_dev]_CFP64.  The system operator, every Krylov vector, dot and scalar stay ComplexF64; the preconditioner narrows its
 * input into the fine level's b, runs the single cycle from zero and widens the result (the widening pass is the copy-out the
 * drivers make anyway; BiCGSTAB's s_hat takes one more vector).  Without a Krylov operator set, As[1] is widened once into the
 * Krylov operator at the first driver call - the Krylov product is never single.  mg_cycle_dev_CFP64 on a CF32 handle is that
 * closure on ComplexF64 device vectors, from zero: x_is_zero = 0 returns MG_ERR_UNSUPPORTED.
 *
 * Refusals.  A _CF32 entry point on a CF64 or FP64 handle, and mg_set_operator_CF64_INT64 / mg_set_relax_CF64 / mg_cycle_CF64 /
 * mg_solve_CF64 / mg_spmv_CF64 / mg_set_operator_FP64_INT64 on a CF32 handle: MG_ERR_STATE.  Not served for a CF32 handle
 * (MG_ERR_UNSUPPORTED): mg_rap_CF64, mg_rap_level_ms_CF64, mg_get_values_CF64, mg_get_relax_CF64, mg_replace_values_CF64 (their
 * _CF32 forms above serve it), mg_set_coarse_dd with a ComplexF64 sweep handle (a ComplexF32 one is served: "Float32 / ComplexF32 Schwarz sweeps"), the K-cycle and Jac-GMRES (served with the option single_kcycle, see mg_set_schedule_CF32),
 * nrhs > 1 in the entry points of this section (blocks: mg_block_cycle_dev_CFP64 and mg_block_bicgstab[_dev]_CFP64 below), and
 * whatever a CF64 handle does not serve. */
int mg_create_CF32(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out);
int mg_set_operator_CF32_INT64(mg_hierarchy* h, long long level, long long which, long long n_rows, long long n_cols,
                               const long long* colptr, const long long* rowval, const float* nzval);
int mg_set_relax_CF32(mg_hierarchy* h, long long level, const float* d, long long n, long long relaxPre, long long relaxPost);
int mg_cycle_CF32(mg_hierarchy* h, const float* b, float* x, long long n, long long nrhs, long long x_is_zero);
int mg_solve_CF32(mg_hierarchy* h, const float* b, float* x, long long n, long long nrhs, double tol, long long maxIter,
                  long long* iters, double* resvec);
int mg_spmv_CF32(mg_hierarchy* h, long long level, long long which, const float* alpha, const float* x, const float* beta,
                 float* y, long long nrhs);

/* ---- blocks of right-hand sides on complex handles: SpMM cycle, block solveMG, block BiCGSTAB, block FGMRES ---------------------
 * What the reference does with size(b,2) > 1 for VAL = ComplexF64: one cycle on the whole block (getMultigridPreconditioner,
 * SolveFuncs.jl:43-63), solveMG with Frobenius norms (l.14-36), KrylovMethods.blockBiCGSTB (l.94-96), KrylovMethods.blockFGMRES (l.130).  k sources then share one pass
 * over every operator instead of streaming it k times.
 *
 * nrhs arrives WITH EACH CALL, 1 <= nrhs <= 16; the handle's own nrhs stays 1 and every entry point above keeps refusing nrhs > 1.
 * The block entry points keep a work set of their own with the handle (level vectors of n_l x nrhs, the widened coarsest pair of a
 * CF32 handle, staging and Krylov blocks), allocated at the first block call, grown when a larger nrhs arrives and released with the
 * handle; the single-vector state is not touched: a single-vector call after a block call gives the bits it gave before.
 *
 * Layout.  Host blocks (B, X, Y of the _CF64 forms and of mg_block_bicgstab_CFP64) are Julia's column-major n x nrhs, interleaved
 * (re, im) doubles; device blocks (the _dev forms) are ROW-MAJOR [n][nrhs] ComplexF64 on a 16-byte boundary - the layout of the
 * real block path.  Products run in csrc/mg_complex.hpp, cx_csr_stream_spmm: the matrix stream of a row block is staged in LDS
 * once and walked by pow2 >= nrhs lanes per row, every (row, column) one lane's sum in stored order - deterministic, and a column's
 * result does not depend on what the other columns hold.
 *
 * mg_block_spmv_CF64: Y = beta*Y + alpha*Op*X on one level (X: n_cols x nrhs, Y: n_rows x nrhs).
 * mg_block_cycle_CF64: one cycle on the block; x_is_zero as for mg_cycle_CF64, a property of the WHOLE block (norm(x) of the
 *   reference).  mg_block_cycle_dev_CFP64: the same on device blocks (x_is_zero 0 or 1), enqueued without a synchronisation; on
 *   a CF32 handle the mixed closure on the whole block (narrow, the single cycle from zero, widen; x_is_zero = 0: MG_ERR_UNSUPPORTED).
 * mg_block_solve_CF64: solveMG with ||.||_F over the block; resvec as for mg_solve_CF64.
 * mg_block_bicgstab[_dev]_CFP64: blockBiCGSTB on the handle's Krylov operator (or As[1]) with one block cycle from zero as M1;
 *   Gram matrices R0^H V, R0^H R (deterministic two-pass sums), k x k complex solves on the host, omega = tr(T^H S)/tr(T^H T).
 *   flag 0 converged, -1 maxIter, -2 breakdown (singular R0^H V, T = 0 or omega = 0), -3 converged on the half step, -9 B = 0 (X = 0);
 *   resvec (up to 2*maxIter + 1 entries, nres of them written): max_j ||r_j|| / ||b_j|| at the start, after every half and full step.
 *   On a CF32 handle every Krylov block stays ComplexF64.
 * mg_block_fgmres[_dev]_CFP64: blockFGMRES(inner) with the arguments of mg_block_fgmres[_dev]_FP64 on the same operator and M: block
 *   modified Gram-Schmidt with H_ij = V_i^H W, Cholesky QR applied twice (pivots at or below 1e-14 G[c][c] dropped), the exact block
 *   least squares on the host after every inner step.  Every Gram operand is read from HBM once, and every Gram matrix but the first
 *   of an inner step is left by the update before it (csrc/mg_complex.hpp: cx_blk_gram_onepass, cx_blk_comb_gram; above 8
 *   columns, where the fused kernel measured slower, the update and the one-pass kernel are two launches); inner step j
 *   synchronises the host j + 3 times.  inner in [1,64] (MG_ERR_INVALID otherwise); work set 2*inner + 2 blocks.  flag 0 converged,
 *   -1 maxIter, -9 B = 0 (X = 0); iters: inner steps in all; resvec (up to maxIter*inner entries): ||xi - H Y||_F / ||B||_F per inner step.
 * Coarsest solve: the dense inverse, the one-workgroup triangular sweeps or the chip-wide factor applier, each on the whole block.
 * Refused: nrhs < 1 (MG_ERR_INVALID), nrhs > 16 (MG_ERR_UNSUPPORTED), a Schwarz sweep as coarsest solve with nrhs > 1
 * (MG_ERR_UNSUPPORTED), an FP64 handle or a handle that is not finalized (MG_ERR_STATE), a CF32 handle in the _CF64 forms
 * (MG_ERR_STATE), a null block, a wrong n, maxIter < 0, a device block off a 16-byte boundary (MG_ERR_INVALID).  A refusal leaves the
 * handle usable.  Not served for complex blocks: PCG, the K-cycle and Jac-GMRES (opt-in: the next section), the sharded forms, HIP graphs.
 * (The _CF64 forms spell their status mg_status, as the re-setup entry points above do.) */
mg_status mg_block_spmv_CF64(mg_hierarchy* h, long long level, long long which, const double* alpha, const double* X,
                             const double* beta, double* Y, long long nrhs);
mg_status mg_block_cycle_CF64(mg_hierarchy* h, const double* B, double* X, long long n, long long nrhs, long long x_is_zero);
mg_status mg_block_solve_CF64(mg_hierarchy* h, const double* B, double* X, long long n, long long nrhs, double tol,
                              long long maxIter, long long* iters, double* resvec);
int mg_block_cycle_dev_CFP64(mg_hierarchy* h, const double* B_dev, double* X_dev, long long n, long long nrhs,
                             long long x_is_zero);
int mg_block_bicgstab_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                            long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
int mg_block_bicgstab_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs,
                                double tol, long long maxIter, long long* iters, long long* flag, double* resvec,
                                long long* nres);
int mg_block_fgmres_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long inner,
                          double tol, long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres);
int mg_block_fgmres_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs,
                              long long inner, double tol, long long maxIter, long long* iters, long long* flag,
                              double* resvec, long long* nres);

/* ---- blocks on K-cycle / Jac-GMRES complex hierarchies, OPT-IN: mg_set_option(h, "kcycle_blocks", 1) before mg_finalize (default 0) -
 * The reference runs FGMRES_relaxation on a block as ONE long vector of length n*nrhs (FGMRES.jl:51-53, 89-97; MGcycle.jl:48-50,
 * 72-76, 96-98): one H, one xi, one t and one break test for the whole block.  With the option every block entry point above serves
 * a handle whose cycle is 'K' and / or whose relaxation type is 1 in that form, 1 <= nrhs <= 16; without it they return
 * MG_ERR_UNSUPPORTED with the messages they had before the option existed.  THE COLUMNS ARE COUPLED: a column's result depends on its
 * neighbours and on their scaling (one t for all), and it is not what the vector entry points give column by column.  A Jac-GMRES
 * cycle is non-linear in its right-hand side: as a preconditioner it belongs under mg_block_fgmres_CFP64, not mg_block_bicgstab_CFP64.
 * Kernels: the GRAM mode of cx_csr_stream_spmm (W = A Z_j as block j of AZ, the next direction d.*W, and per row block the partial
 * sums over all its rows and columns of the vector form's 2 j + 3 scalars: lane registers, wavefront shuffles, LDS, no atomics, the
 * same bits on every run).  One host synchronisation per relaxation and one per K step for the WHOLE block - the vector form's counts.
 * Work set (with the block work set, grown with nrhs): per Jac-GMRES level 2*max(relaxPre, relaxPost) blocks of n_l x nrhs, per
 * level from 2 on with 'K' four blocks.  A CF32 handle is served when its option single_kcycle is set as well (the mixed complex128
 * closure of the block entry points); a GMRES coarsest solve when coarse_gmres_blocks is set as well.  Still MG_ERR_UNSUPPORTED: Vanka
 * with 'K' on a block, a Schwarz coarsest solve on a block, nrhs > 16, more than 8 directions, FP64 handles, the sharded forms.
 * mg_block_fgmres_relax_CF64 / _CF32: one such relaxation on As[level] and relaxPrecs[level] from host blocks, X += sum_j t_j Z_j for
 * the residual block R0.  Both take ComplexF64 column-major n x nrhs host blocks; the CF32 form narrows on the device and returns X,
 * Z_out and AZ_out widened, which is exact.  1 <= level < nlevels, 1 <= inner <= 8.  H_out, xi_out, rnorms_out, used_out as for
 * mg_fgmres_relax_CF64; Z_out / AZ_out (may be NULL) receive the bases as n x nrhs x inner (block j a column-major n x nrhs block;
 * the leading `used` blocks enter X).  Without the option: MG_ERR_UNSUPPORTED. */
mg_status mg_block_fgmres_relax_CF64(mg_hierarchy* h, long long level, const double* R0, double* X, long long n, long long nrhs,
                                     long long inner, double tol, double* H_out, double* xi_out, double* rnorms_out,
                                     long long* used_out, double* Z_out, double* AZ_out);
mg_status mg_block_fgmres_relax_CF32(mg_hierarchy* h, long long level, const double* R0, double* X, long long n, long long nrhs,
                                     long long inner, double tol, double* H_out, double* xi_out, double* rnorms_out,
                                     long long* used_out, double* Z_out, double* AZ_out);

const char* mg_last_error(void);
const char* mg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MGVCYCLE_H */
