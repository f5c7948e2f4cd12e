// mg_formats.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// Host <-> device block transfer, format construction at upload / finalize (row classes, patterns, tiles, marching forms, band form, windows), numeric RAP support, scratch allocation.
namespace {
// ---- host <-> device block transfer (column-major host <-> row-major device) --------------------
int upload_block(mg_hierarchy* h, const double* host, double* dev, long long n, long long nrhs) {
  const size_t bytes = sizeof(double) * (size_t)n * (size_t)nrhs;
  if (nrhs == 1) {
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->play->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(h->stage_t.p, host, bytes, hipMemcpyHostToDevice, h->play->stream));
    hipLaunchKernelGGL(mgk::colmajor_to_rowmajor, dim3(grid_for(n * nrhs)), dim3(mgk::BLK), 0, h->play->stream,
                       h->stage_t.p, dev, n, (int)nrhs);
    HIP_TRY(hipGetLastError());
  }
  return MG_OK;
}
int download_block(mg_hierarchy* h, const double* dev, double* host, long long n, long long nrhs) {
  const size_t bytes = sizeof(double) * (size_t)n * (size_t)nrhs;
  if (nrhs == 1) {
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->play->stream));
  } else {
    hipLaunchKernelGGL(mgk::rowmajor_to_colmajor, dim3(grid_for(n * nrhs)), dim3(mgk::BLK), 0, h->play->stream,
                       dev, h->stage_t.p, n, (int)nrhs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, h->stage_t.p, bytes, hipMemcpyDeviceToHost, h->play->stream));
  }
  HIP_TRY(spin_sync(h->play->stream));
  return MG_OK;
}

// L2-tiled processing order of the row blocks of M, whose rows form an x-fastest n1 x n2 x n3 grid.
// In natural order two blocks that gather from the same z-neighbour planes are a whole plane apart; when
// three planes of the gathered vector (x nrhs) exceed an XCD's 4 MiB L2 those gathers miss.  Walking the
// grid in y-tiles (all z for T consecutive y-lines, then the next tile) brings the reuse distance down to
// ~2T lines.  Pure scheduling: every block computes exactly what it computed before.
int build_schedule_for(Csr& M, const long long grid[3], long long nrhs, const std::vector<int>& h_blk, int nb,
                       DevBuf<int>& sched, bool& has);
// Plane tiles for csr_rowclass_tile_spmv: needs the row-class form without a first-column stream and a grid hint
// whose plane size divides the row count; the halo is what the most frequent class reaches inside a plane.
int build_tile(Csr& A, const long long grid[3]) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  A.rc_tile = false;
  if (!A.has_rc || !A.rc_implicit || A.h_rc_ptr.empty()) return MG_OK;
  if (A.opt.no_tile) return MG_OK;
  if (grid[0] < 1 || grid[1] < 1 || grid[2] < 2 || grid[0] * grid[1] * grid[2] != (A.regular_cols >= 0 ? A.regular_cols : A.n_rows)) return MG_OK;
  const long long P = grid[0] * grid[1];
  if (P < mgk::RT_CR / 2 || A.n_rows + (mgk::RT_NP + 2) * P >= (1LL << 31) - 1) return MG_OK;   // int32 row arithmetic in the kernel
  // 1024 rows of a plane per workgroup; levels whose 1024-row tiles number fewer than tile_min_wg take 256-row tiles (4 x
  // the workgroups, a quarter of the threads each) if THOSE fill the chip - else the lane kernel serves the level
  long long CRt = mgk::RT_CR;
  {
    const long long groups = (grid[2] + mgk::RT_NP - 1) / mgk::RT_NP;
    if (((P + CRt - 1) / CRt) * groups < A.opt.tile_min_wg && !A.opt.no_tile_small && ((P + 255) / 256) * groups >= A.opt.tile_min_wg) CRt = 256;
  }
  auto split = [&](long long sh, long long& dz, long long& rest) {
    dz = (sh >= 0) ? (sh + P / 2) / P : -((-sh + P / 2) / P);
    rest = sh - dz * P;
  };
  const int cm = A.rc_major;
  {
    const long long min_len = A.opt.stage_min_len;    // as for the window kernel
    if (A.h_rc_ptr[(size_t)cm + 1] - A.h_rc_ptr[(size_t)cm] < min_len) return MG_OK;
  }
  long long halo = 1;
  for (int k = A.h_rc_ptr[(size_t)cm]; k < A.h_rc_ptr[(size_t)cm + 1]; ++k) {
    long long dz, rest;
    split((long long)A.h_rc_delta[(size_t)cm] + A.h_rc_off[(size_t)k], dz, rest);
    if (dz < -1 || dz > 1) return MG_OK;
    halo = std::max(halo, rest < 0 ? -rest : rest);
  }
  const long long SL = CRt + 2 * halo;
  if ((mgk::RT_NP + 2) * SL * 8 > 80 * 1024) return MG_OK;   // two workgroups per CU
  std::vector<int> lbs(A.h_rc_off.size(), -1);
  for (size_t c = 0; c + 1 < A.h_rc_ptr.size(); ++c)
    for (int k = A.h_rc_ptr[c]; k < A.h_rc_ptr[c + 1]; ++k) {
      long long dz, rest;
      split((long long)A.h_rc_delta[c] + A.h_rc_off[(size_t)k], dz, rest);
      if (dz >= -1 && dz <= 1 && rest >= -halo && rest <= halo) lbs[(size_t)k] = (int)((dz + 1) * SL + rest + halo);
    }
  MG_TRY(A.rt_lb.alloc(lbs.size()));
  HIP_TRY(hipMemcpy(A.rt_lb.p, lbs.data(), lbs.size() * sizeof(int), hipMemcpyHostToDevice));
  A.rt_P = (int)P;
  A.rt_nplanes = (int)grid[2];
  A.rt_halo = (int)halo;
  A.rt_lane = !A.opt.no_tile_lane && std::all_of(lbs.begin(), lbs.end(), [](int v) { return v >= 0; }) &&
              A.rc_ncls * (long long)A.rc_maxlen <= mgk::RT_LCAP &&
              (mgk::RT_NP + 2) * SL * 8 + A.rc_ncls * (long long)A.rc_maxlen * 16 + A.rc_ncls * 8 <= 80 * 1024;
  A.rt_cr = (int)CRt;
  A.rt_chunks = (int)((P + CRt - 1) / CRt);
  A.rt_nblocks = (int)(((grid[2] + mgk::RT_NP - 1) / mgk::RT_NP) * A.rt_chunks);
  {
    // 4096 rows per workgroup: a level that yields fewer workgroups than the chip has CUs is latency-bound and runs
    // faster on the 256/512-row kernels (C2 level 3, 65^3 rows: 85 workgroups, 26 us against 17 us)
    if (A.rt_nblocks < A.opt.tile_min_wg) return MG_OK;
  }
  A.rc_tile = true;
  return MG_OK;
}

// z-marching form (csr_rowclass_march_spmv): same preconditions as the plane tiles; the workgroups are one balanced
// round of the resident slots (2 per CU), each with at least 8 planes to walk.
int build_march(Csr& A, const long long grid[3]) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  A.rc_march = false;
  if (!A.has_rc || !A.rc_implicit || A.h_rc_ptr.empty() || A.opt.no_march) return MG_OK;
  // (a padded local operator of a sharded level: the grid is the owned box = its first regular_cols rows)
  if (grid[0] < 1 || grid[1] < 1 || grid[2] < 2 || grid[0] * grid[1] * grid[2] != (A.regular_cols >= 0 ? A.regular_cols : A.n_rows)) return MG_OK;
  const long long P = grid[0] * grid[1];
  if (P < 64 || A.n_rows + 4 * P >= (1LL << 31) - 1) return MG_OK;   // int32 row arithmetic in the kernel
  auto split = [&](long long sh, long long& dz, long long& rest) {
    dz = (sh >= 0) ? (sh + P / 2) / P : -((-sh + P / 2) / P);
    rest = sh - dz * P;
  };
  const int cm = A.rc_major;
  if (A.h_rc_ptr[(size_t)cm + 1] - A.h_rc_ptr[(size_t)cm] < A.opt.stage_min_len) return MG_OK;
  long long halo = 1;
  for (int k = A.h_rc_ptr[(size_t)cm]; k < A.h_rc_ptr[(size_t)cm + 1]; ++k) {
    long long dz, rest;
    split((long long)A.h_rc_delta[(size_t)cm] + A.h_rc_off[(size_t)k], dz, rest);
    if (dz < -1 || dz > 1) return MG_OK;
    halo = std::max(halo, rest < 0 ? -rest : rest);
  }
  if (halo > 510) return MG_OK;   // one 16-byte pair per thread covers the slab
  if (A.rc_ncls > mgk::RM_NCLS || A.rc_entries > mgk::RM_DCAP) return MG_OK;   // the dictionary lives in LDS
  if (A.rc_maxlen > A.opt.march_max_len) return MG_OK;
  std::vector<int> lbs(A.h_rc_off.size(), -1);
  for (size_t c = 0; c + 1 < A.h_rc_ptr.size(); ++c)
    for (int k = A.h_rc_ptr[c]; k < A.h_rc_ptr[c + 1]; ++k) {
      long long dz, rest;
      split((long long)A.h_rc_delta[c] + A.h_rc_off[(size_t)k], dz, rest);
      if (dz >= -1 && dz <= 1 && rest >= -halo && rest <= halo) lbs[(size_t)k] = (int)(((rest + halo) << 2) | (dz + 1));
      else return MG_OK;   // an entry outside the staged shifts (not a grid operator / wrong hint): plane tiles + gathers
    }
  const long long chunks = (P + mgk::RM_C - 1) / mgk::RM_C;
  const long long items = chunks * grid[2];
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const long long nb = std::max<long long>(1, std::min<long long>(A.opt.march_wg_per_cu * ncu, items / 8));
  if (nb < A.opt.march_min_wg) return MG_OK;   // small levels: latency-bound, the other kernels serve them
  MG_TRY(A.rm_lb.alloc(lbs.size()));
  HIP_TRY(hipMemcpy(A.rm_lb.p, lbs.data(), lbs.size() * sizeof(int), hipMemcpyHostToDevice));
  A.rm_P = (int)P;
  A.rm_nplanes = (int)grid[2];
  A.rm_halo = (int)halo;
  A.rm_chunks = (int)chunks;
  A.rm_nblocks = (int)nb;
  A.rc_march = true;
  // two stages per pass (sweep + residual): no exception rows, x slab of RM_C + 4*halo entries in two 16-byte pairs per
  // thread, ring of 4 x slabs + 4 t slabs + dictionary within the 160 KB of LDS; one workgroup per CU
  A.rc_march2 = false;
  A.rm2_nblocks = (int)std::max<long long>(1, std::min<long long>(ncu, items / 8));
  if (!A.opt.no_march2 && A.rc_nexc == 0 && A.regular_cols < 0 && 2 * halo <= mgk::RM_C && march2_lds_bytes((int)halo) <= 160 * 1024 - 256 &&
      A.rm2_nblocks >= std::min<long long>(A.opt.march_min_wg, ncu))
    A.rc_march2 = true;
  return MG_OK;
}
int build_march3(Csr& A, const long long grid[3]);
// every staged form of a level's A that depends on the grid hint and on the classes
int build_march27(Csr& A, const long long grid[3]);
int build_marchr(Csr& R, const long long gf[3], const long long gc[3]);
int build_staged(Csr& A, const long long grid[3]) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  MG_TRY(build_tile(A, grid));
  MG_TRY(build_march(A, grid));
  MG_TRY(build_march3(A, grid));
  return build_march27(A, grid);
}

// 2-D tile form of the two-stage pass (csr_rowclass_march3_spmv): the operator must be a grid operator of z-star classes -
// per class at most one entry in plane z-1 (the first) and one in plane z+1 (the last), both at the row's own in-plane
// position, and at most RM3_NIP in-plane entries (dy, dx), |dy|, |dx| <= 1 - whose class ids factor as
// cls(x, y, z) = tab[cz[z]][cy[y]][cx[x]] (found by hashing the three families of grid slices, then VERIFIED row by row).
// Tile geometry: the stage-1 region is WX = TX + 2 columns wide, an NT-thread workgroup holds SY = NT / WX lines of it per
// slot pass and K1 passes, so TY = K1*SY - 2; threads per workgroup (1024 with K1 <= 3: 128 registers per lane; 768 with
// K1 <= 4: 168), tiles per line and K1 are chosen by an estimate of the bytes filled per row (halo, run ends, the partial
// cache lines at both ends of a tile's line segments), within the LDS (3 x slabs + 2 t slabs + tables <= 160 KB) and the
// 16-byte pairs a lane can load per slab.  Schedule: lockstep (tiles x segments of planes = about one workgroup per CU, all
// tiles of a segment on one XCD) when that keeps >= 85 % of the balanced schedule's parallel efficiency.
struct M3Ent { int dz, dy, dx; };
int build_march3_impl(Csr& A, const long long grid[3], const unsigned short* cl, size_t ncls,
                      const std::vector<std::vector<M3Ent>>& ents, bool var, bool canon = false);
int build_band(Csr& A, const long long grid[3]);
int band_refill(Csr& A) {
  const int NS = mgk::RM3_NIP + 2;
  const unsigned nb = (unsigned)((A.n_rows + mgk::BLK - 1) / mgk::BLK);
  hipLaunchKernelGGL(mgk::band_fill, dim3(nb), dim3(mgk::BLK), 0, nullptr, A.rowptr.p, A.val.p,
                     A.vb_cls.p, A.vb_slot.p, NS, A.vband.p, A.vstride, (int)A.n_rows);
  HIP_TRY(hipGetLastError());
  // symmetric values (div sigma grad: G' diag(sigma) G)?  Then the lower entries are read from the upper ones of the neighbour row
  A.band_sym = false;
  if (A.band_canon && !A.opt.no_band_sym) {
    if (A.vb_bad.n != 1) MG_TRY(A.vb_bad.alloc(1));
    HIP_TRY(hipMemsetAsync(A.vb_bad.p, 0, sizeof(int), nullptr));
    hipLaunchKernelGGL(mgk::band_sym_check, dim3(nb), dim3(mgk::BLK), 0, nullptr, A.vband.p, A.vstride, (int)A.n_rows, A.rm3.n1, A.rm3.P, A.vb_bad.p);
    HIP_TRY(hipGetLastError());
    int bad = 1;
    HIP_TRY(hipMemcpy(&bad, A.vb_bad.p, sizeof(int), hipMemcpyDeviceToHost));
    A.band_sym = bad == 0;
  }
  HIP_TRY(hipDeviceSynchronize());
  for (int k = 0; k < NS; ++k) A.rm3.vsrc[k] = (long long)k * A.vstride;
  if (A.band_sym) {
    A.rm3.vsrc[0] = 6 * A.vstride - A.rm3.P;
    A.rm3.vsrc[1] = 5 * A.vstride - A.rm3.n1;
    A.rm3.vsrc[2] = 4 * A.vstride - 1;
  }
  return MG_OK;
}
int build_march3(Csr& A, const long long grid[3]) {
  // band form, same pattern (the pattern of a set operator never changes: mg_replace_values / mg_rap keep it), same grid: only
  // the values moved - one kernel refills the planar arrays from the CSR values
  if (!A.has_rc && A.rm3_var && A.rc_march3 && A.rm3.n1 == grid[0] && A.rm3.n2 == grid[1] && A.rm3.nplanes == grid[2] && !A.opt.no_band &&
      !A.opt.no_march3 && !A.opt.no_march2 && !A.opt.no_march)
    return band_refill(A);
  A.rc_march3 = false;
  A.rc_march4 = false;
  A.rm3_var = false;
  A.vband.release();
  if (!A.has_rc) return build_band(A, grid);
  if (!A.has_rc || !A.rc_implicit || A.h_rc_ptr.empty() || A.opt.no_march3 || A.opt.no_march2 || A.opt.no_march) return MG_OK;
  // a box operator of a sharded level (regular_cols >= 0): the grid is the owned box = its first regular_cols rows; the rows
  // that read the halo are exception rows (class 0xFFFF) and stay so here
  const bool box = A.regular_cols >= 0;
  const long long nreg = box ? A.regular_cols : A.n_rows;
  if (A.rc_nexc != 0 && !box) return MG_OK;
  A.rc_exc2.release();
  A.rc_nexc2 = 0;
  const long long n1 = grid[0], n2 = grid[1], n3 = grid[2];
  if (n1 < 4 || n2 < 4 || n3 < 3 || n1 * n2 * n3 != nreg) return MG_OK;
  if (n1 > 65535 || n2 > 65535 || n3 > 65535 || A.h_cls.size() != (size_t)A.n_rows) return MG_OK;
  const long long P = n1 * n2;
  if (A.n_rows + 4 * P >= (1LL << 31) - 1) return MG_OK;   // int32 row arithmetic in the kernel
  const size_t ncls = A.h_rc_ptr.size() - 1;
  if (ncls > (size_t)mgk::RM3_NCLS) return MG_OK;
  // ---- classes: decompose every column shift into (dz, dy, dx) ------------------------------------------------------------
  using Ent = M3Ent;
  std::vector<std::vector<Ent>> ents(ncls);
  for (size_t c = 0; c < ncls; ++c) {
    int nip = 0;
    const int k0 = A.h_rc_ptr[c], k1 = A.h_rc_ptr[c + 1];
    for (int k = k0; k < k1; ++k) {
      const long long sh = (long long)A.h_rc_delta[c] + A.h_rc_off[(size_t)k];
      const long long dz = (sh >= 0) ? (sh + P / 2) / P : -((-sh + P / 2) / P);
      const long long rest = sh - dz * P;
      const long long dy = (rest >= 0) ? (rest + n1 / 2) / n1 : -((-rest + n1 / 2) / n1);
      const long long dx = rest - dy * n1;
      if (dz < -1 || dz > 1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) return MG_OK;
      if (dz != 0 && (dy != 0 || dx != 0)) return MG_OK;           // not a z-star
      if (dz == -1 && k != k0) return MG_OK;                       // the z-1 entry comes first ...
      if (dz == 1 && k != k1 - 1) return MG_OK;                    // ... the z+1 entry last (ascending columns)
      if (dz == 0 && ++nip > mgk::RM3_NIP) return MG_OK;
      ents[c].push_back({(int)dz, (int)dy, (int)dx});
    }
  }
  return build_march3_impl(A, grid, A.h_cls.data(), ncls, ents, false);
}

// Band form (csr_rowclass_march3_spmv<..., VAR = true>) of a grid operator that has NO row classes because its coefficients
// differ from row to row: classes of the STRUCTURE (the sorted list of column shifts of a row), which must be z-stars and
// factor as a product map exactly like the value classes of build_march3, and the values re-laid as 7 planar arrays
// (slot 0 the z-1 entry, 1..5 the in-plane entries in stored order, 6 the z+1 entry; 0 where a row has none).  Built from the
// device's CSR arrays (copied back once), re-built whenever build_staged runs again (new values: replaceMatrixInHierarchy).
int build_band(Csr& A, const long long grid[3]) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  if (A.opt.no_band || A.opt.no_march3 || A.opt.no_march2 || A.opt.no_march || A.regular_cols >= 0) return MG_OK;
  const long long n1 = grid[0], n2 = grid[1], n3 = grid[2];
  if (n1 < 4 || n2 < 4 || n3 < 3 || n1 * n2 * n3 != A.n_rows || A.n_cols != A.n_rows) return MG_OK;
  if (A.n_rows < A.opt.band_min_rows || A.max_row_nnz > mgk::RM3_NIP + 2) return MG_OK;
  const long long P = n1 * n2, n = A.n_rows;
  std::vector<int> rp((size_t)n + 1), ci((size_t)std::max<long long>(A.nnz, 1));
  HIP_TRY(hipMemcpy(rp.data(), A.rowptr.p, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (A.nnz > 0) HIP_TRY(hipMemcpy(ci.data(), A.colidx.p, (size_t)A.nnz * sizeof(int), hipMemcpyDeviceToHost));
  // ---- structure classes: rows with the same list of shifts --------------------------------------------------------------
  std::vector<unsigned short> cl((size_t)n);
  std::vector<std::vector<long long>> shifts;          // per class
  std::unordered_map<unsigned long long, std::vector<int>> byhash;
  for (long long i = 0; i < n; ++i) {
    const int k0 = rp[(size_t)i], k1 = rp[(size_t)i + 1];
    unsigned long long hsh = 0x9E3779B97F4A7C15ULL * (unsigned long long)(k1 - k0 + 1);
    for (int k = k0; k < k1; ++k) {
      hsh ^= (unsigned long long)((long long)ci[(size_t)k] - i) + 0x9E3779B97F4A7C15ULL + (hsh << 6) + (hsh >> 2);
    }
    std::vector<int>& cand = byhash[hsh];
    int found = -1;
    for (int c : cand) {
      const std::vector<long long>& sh = shifts[(size_t)c];
      if ((int)sh.size() != k1 - k0) continue;
      bool same = true;
      for (int k = k0; k < k1 && same; ++k) same = sh[(size_t)(k - k0)] == (long long)ci[(size_t)k] - i;
      if (same) { found = c; break; }
    }
    if (found < 0) {
      if (shifts.size() >= (size_t)mgk::RM3_NCLS) return MG_OK;
      std::vector<long long> sh((size_t)(k1 - k0));
      for (int k = k0; k < k1; ++k) sh[(size_t)(k - k0)] = (long long)ci[(size_t)k] - i;
      found = (int)shifts.size();
      shifts.push_back(sh);
      cand.push_back(found);
    }
    cl[(size_t)i] = (unsigned short)found;
  }
  const size_t ncls = shifts.size();
  std::vector<std::vector<M3Ent>> ents(ncls);
  for (size_t c = 0; c < ncls; ++c) {
    int nip = 0;
    const size_t len = shifts[c].size();
    for (size_t k = 0; k < len; ++k) {
      const long long sh = shifts[c][k];
      if (k > 0 && sh <= shifts[c][k - 1]) return MG_OK;             // (ascending columns)
      const long long dz = (sh >= 0) ? (sh + P / 2) / P : -((-sh + P / 2) / P);
      const long long rest = sh - dz * P;
      const long long dy = (rest >= 0) ? (rest + n1 / 2) / n1 : -((-rest + n1 / 2) / n1);
      const long long dx = rest - dy * n1;
      if (dz < -1 || dz > 1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) return MG_OK;
      if (dz != 0 && (dy != 0 || dx != 0)) return MG_OK;             // not a z-star
      if (dz == -1 && k != 0) return MG_OK;
      if (dz == 1 && k != len - 1) return MG_OK;
      if (dz == 0 && ++nip > mgk::RM3_NIP) return MG_OK;
      ents[c].push_back({(int)dz, (int)dy, (int)dx});
    }
  }
  // canonical slots where every class is a 7-point star: slot = the entry's place in (-z, -y, -x, diagonal, +x, +y, +z) whatever the
  // row holds (0 where it has none; the records then carry the five in-plane offsets in that order) - what the symmetric reads need
  auto star_slot = [](const M3Ent& t) { return t.dz == -1 ? 0 : t.dz == 1 ? 6 : (t.dy == -1 && t.dx == 0) ? 1 : (t.dy == 0 && t.dx == -1) ? 2 :
                                               (t.dy == 0 && t.dx == 0) ? 3 : (t.dy == 0 && t.dx == 1) ? 4 : (t.dy == 1 && t.dx == 0) ? 5 : -1; };
  bool canon = mgk::RM3_NIP == 5;
  for (size_t c = 0; c < ncls && canon; ++c)
    for (const M3Ent& t : ents[c]) canon = canon && star_slot(t) >= 0;
  MG_TRY(build_march3_impl(A, grid, cl.data(), ncls, ents, true, canon));
  if (!A.rc_march3) return MG_OK;
  // ---- the values as planar slots: class ids + slot table to the device, one kernel fills (and later refills) the arrays ------
  // (every slot is followed by at least a plane of zeros: the symmetric reads of row r - P / r - n1 / r - 1 land there for the first rows)
  const long long vstride = ((n + 15) & ~15LL) + ((P + 15) & ~15LL);
  const int NS = mgk::RM3_NIP + 2;
  std::vector<int> slot(ncls * (size_t)NS, 0);
  for (size_t c = 0; c < ncls; ++c) {
    int nip = 0, e = 0;
    for (const M3Ent& t : ents[c]) slot[c * (size_t)NS + (size_t)e++] = canon ? star_slot(t) : (t.dz == -1 ? 0 : t.dz == 1 ? NS - 1 : 1 + nip++);
  }
  A.band_canon = canon;
  MG_TRY(A.vband.alloc((size_t)NS * (size_t)vstride));
  MG_TRY(A.vb_cls.alloc(cl.size()));
  MG_TRY(A.vb_slot.alloc(slot.size()));
  HIP_TRY(hipMemset(A.vband.p, 0, A.vband.bytes()));
  HIP_TRY(hipMemcpy(A.vb_cls.p, cl.data(), cl.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(A.vb_slot.p, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
  A.vstride = vstride;
  A.rm3.vband = A.vband.p;
  A.rm3.vstride = vstride;
  MG_TRY(band_refill(A));
  A.rm3_var = true;
  A.band_ncls = (long long)ncls;
  return MG_OK;
}

// Four-stage pass of the solve loop (csr_rowclass_march4_spmv) on an operator the two-stage tile form serves: the same
// classes and product map; the in-plane entries of every class must lie in {-y, -x, 0, +x, +y} (the records carry values
// in that canonical order, no offsets), at most 4 z-classes and 255 classes (a lane packs its rows' class ids per
// z-class into one register), relaxPrec constant per class.  Tile geometry of its own - the stage-1 region is WX = TX + 6
// columns wide (three rings around the core), a lane owns K1 vertically adjacent rows, SY lanes per column:
// TY <= K1*SY - 6; 3 slabs of x and 2 each of t, xn, t', all K1*SY + 2 lines, within the 160 KB of LDS; lockstep schedule
// (tiles x segments of planes = at most one workgroup per CU).
int build_march4(Csr& A, const std::vector<mgk::M3Class>& recs3, const std::vector<std::vector<M3Ent>>& ents, int ncx, int ncy, int ncz,
                 size_t map_bytes, int ncu, const unsigned short* cy) {
  A.rc_march4 = false;
  if (A.opt.no_march4 || !A.rc_has_d) return MG_OK;
  const long long n1 = A.rm3.n1, n2 = A.rm3.n2, n3 = A.rm3.nplanes, P = n1 * n2;
  const size_t ncls = recs3.size();
  if (n3 < 8 || ncz > 4 || ncls > 255 || (size_t)A.rc_ncls != ncls) return MG_OK;
  if (A.n_rows + 8 * P >= (1LL << 31) - 1) return MG_OK;   // int32 row arithmetic in the kernel
  // ---- records in canonical form ---------------------------------------------------------------------------------------------
  std::vector<double> dcls(ncls);
  HIP_TRY(hipMemcpy(dcls.data(), A.rc_d.p, ncls * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<mgk::M4Class> recs(ncls);
  for (size_t c = 0; c < ncls; ++c) {
    mgk::M4Class q{};
    q.v_lo = recs3[c].v_lo;
    q.v_hi = recs3[c].v_hi;
    q.d = dcls[c];
    int nip = 0, last = -1;
    for (const M3Ent& t : ents[c]) {
      if (t.dz != 0) continue;
      int slot = -1;
      if (t.dy == -1 && t.dx == 0) slot = 0;
      else if (t.dy == 0 && t.dx == -1) slot = 1;
      else if (t.dy == 0 && t.dx == 0) slot = 2;
      else if (t.dy == 0 && t.dx == 1) slot = 3;
      else if (t.dy == 1 && t.dx == 0) slot = 4;
      if (slot < 0 || slot <= last) return MG_OK;       // a diagonal in-plane entry, or not in ascending order: two passes
      last = slot;
      q.v[slot] = recs3[c].v[nip++];
    }
    recs[c] = q;
  }
  const long long lds_cap = 160 * 1024 - 1024;
  (void)map_bytes;   // (march3 stages the whole map; here only cz | tab go to LDS)
  const size_t dict_bytes = ncls * sizeof(mgk::M4Class) + ((((size_t)n3 + (size_t)ncx * ncy * ncz) * 2 + 15) & ~(size_t)15);
  struct Geo { long long NT, tilesx, TX, TY, tilesy, WX, SY, NPL, pitch, LY, LYA, K1, NPM, nb, segs, seglen; size_t lds; double fill, cost; };
  Geo best{};
  bool have = false;
  const long long want_nt = A.opt.march4_nt != 0 ? A.opt.march4_nt : 1024;
  const long long want_k1 = A.opt.march4_k1 != 0 ? A.opt.march4_k1 : (want_nt == 1024 ? 2 : want_nt == 768 ? 3 : 4);
  for (long long NT : {1024LL, 768LL, 512LL}) {
    if (NT != want_nt) continue;
    const long long K1 = want_k1, NPM = (NT == 512 || (NT == 768 && K1 == 4)) ? 3 : 2;
    if (!((NT == 1024 && K1 == 2) || (NT == 768 && (K1 == 3 || K1 == 4)) || (NT == 512 && K1 == 4))) continue;   // (instantiated shapes)
    for (long long tilesx = 1; tilesx <= std::max<long long>({1, n1 / 16, A.opt.march4_tiles_x}); ++tilesx) {
      if (A.opt.march4_tiles_x > 0 && tilesx != A.opt.march4_tiles_x) continue;
      Geo g{};
      g.NT = NT; g.K1 = K1; g.NPM = NPM; g.tilesx = tilesx;
      g.TX = (n1 + tilesx - 1) / tilesx;
      g.WX = g.TX + 6;
      if (g.WX > NT / 2) continue;
      g.NPL = (g.TX + 2 * mgk::RM4_G + 2) / 2;
      g.pitch = 0;
      for (long long pt : {48LL, 64LL, 80LL})      // (the instantiated pitches)
        if (g.pitch == 0 && pt >= 2 * g.NPL) g.pitch = pt;
      if (g.pitch == 0) continue;
      // the tallest tile the lanes, the pair loads and the LDS allow
      long long SY = NT / g.WX;
      // (a tile row's strips may be shifted by up to K1 - 1 lines: that many more lines per column)
      auto fits = [&](long long sy) {
        const long long ty = std::min<long long>(K1 * sy - 6 - (K1 - 1), n2);
        return ty >= 2 && (ty + 8 + K1 - 1) * g.NPL <= NPM * NT && (long long)((size_t)9 * (size_t)(K1 * sy + 2) * (size_t)g.pitch * 8 + dict_bytes) <= lds_cap;
      };
      while (SY >= 1 && !fits(SY)) --SY;
      if (SY < 1) continue;
      long long TY = std::min<long long>(K1 * SY - 6 - (K1 - 1), n2);
      if (A.opt.march4_ty_max > 0) TY = std::min<long long>(TY, A.opt.march4_ty_max);
      g.tilesy = (n2 + TY - 1) / TY;
      g.TY = (n2 + g.tilesy - 1) / g.tilesy;                        // equal tiles
      g.SY = (g.TY + 6 + (K1 - 1) + K1 - 1) / K1;                   // strips a column needs
      g.LY = g.TY + 8 + (K1 - 1);
      g.LYA = K1 * g.SY + 2;
      g.lds = (size_t)9 * (size_t)g.LYA * (size_t)g.pitch * 8 + dict_bytes;
      const long long tiles = g.tilesx * g.tilesy, slots = ncu;
      // Segments per tile: one round of the chip's workgroup slots (one per CU) where the tiles leave room for it; a plane
      // with more tiles than that (513-node lines: 196) takes several rounds of shorter segments - the hardware starts the next
      // workgroup on a CU as one ends, and rounds x (planes + 6) is what a CU works through.
      long long S = 1, rounds = (tiles + slots - 1) / slots;
      {
        double bestr = 0.0;
        for (long long sc = 1; sc <= std::max<long long>(1, n3 / 8); ++sc) {
          if (A.opt.march4_segs > 0 && sc != A.opt.march4_segs) continue;
          const long long lz = (n3 + sc - 1) / sc, rd = (tiles * sc + slots - 1) / slots;
          const double c = (double)rd * (double)(lz + 6);
          if (bestr == 0.0 || c < bestr) { bestr = c; S = sc; rounds = rd; }
        }
      }
      const long long Lz = (n3 + S - 1) / S;
      const double eff = ((double)n3 / (double)(S * Lz)) * ((double)(tiles * S) / (double)(rounds * slots));
      g.segs = S; g.seglen = Lz; g.nb = tiles * S;
      // Cost of a geometry = what ONE workgroup takes (they all run side by side, one per CU): iterations x time per iteration.
      // Measured on 257^3 (profiles/r04_march4_ab.md: nine geometries at 1024 threads): an iteration costs 1.2 us + 1.05 ns per
      // row of the stage-1 region, whatever the tile's shape - so the run length (planes of a segment + 6) decides: the most
      // segments the tiles leave room for, tiles as large as the lanes allow.  (`fill`, kept for the reports: bytes per row.)
      const double core = (double)g.TX * (double)g.TY, R = (double)Lz;
      const double waste = (double)(g.tilesx * g.TX) * (double)(g.tilesy * g.TY) / (double)P;
      const double fx = 8.0 * (double)((g.TX + 8) * (g.TY + 8)) / core * (1.0 + 8.0 / R);
      const double fb = 8.0 * (double)((g.TX + 6) * (g.TY + 6)) / core * (1.0 + 6.0 / R);
      g.fill = (waste * (fx + fb) + 16.0) / eff;
      g.cost = (double)rounds * ((double)Lz + 6.0) * (1.2 + 1.05e-3 * (double)((g.TX + 6) * (g.TY + 6)));
      if (!have || g.cost < best.cost) {
        best = g;
        have = true;
      }
    }
  }
  if (!have) return MG_OK;
  if (best.nb < std::min<long long>(A.opt.march_min_wg, (long long)ncu * 3 / 4)) return MG_OK;   // small levels: latency-bound
  // ---- strip shift per tile row: no strip of K1 lines may hold (live) rows of different y-classes ---------------------------------
  std::vector<int> ysh((size_t)best.tilesy, -1);
  for (long long ty = 0; ty < best.tilesy; ++ty) {
    for (long long sh = 0; sh < best.K1 && ysh[(size_t)ty] < 0; ++sh) {
      bool ok = true;
      for (long long j = 0; j < best.SY && ok; ++j) {
        int seen = -1;
        for (long long r = 0; r < best.K1 && ok; ++r) {
          const long long yc = best.K1 * j + r - sh, gy = ty * best.TY - 3 + yc;
          if (yc < 0 || yc >= best.TY + 6 || gy < 0 || gy >= n2) continue;
          if (seen < 0) seen = cy[gy];
          else if (seen != cy[gy]) ok = false;
        }
      }
      if (ok) ysh[(size_t)ty] = (int)sh;
    }
    if (ysh[(size_t)ty] < 0) return MG_OK;      // lines of different classes inside every strip layout: two passes
  }
  MG_TRY(A.rm4_ysh.alloc(ysh.size()));
  HIP_TRY(hipMemcpy(A.rm4_ysh.p, ysh.data(), ysh.size() * sizeof(int), hipMemcpyHostToDevice));
  MG_TRY(A.rm4_cls.alloc(ncls));
  HIP_TRY(hipMemcpy(A.rm4_cls.p, recs.data(), ncls * sizeof(mgk::M4Class), hipMemcpyHostToDevice));
  mgk::March4Dev T{};
  T.cls = A.rm4_cls.p;
  T.ysh = A.rm4_ysh.p;
  T.cmap = A.rm3_cmap.p;
  T.ncx = ncx; T.ncy = ncy; T.ncz = ncz; T.ntab = ncx * ncy * ncz;
  T.n1 = (int)n1; T.n2 = (int)n2; T.nplanes = (int)n3; T.P = (int)P;
  T.TX = (int)best.TX; T.TY = (int)best.TY; T.tiles_x = (int)best.tilesx; T.tiles_y = (int)best.tilesy;
  T.WX = (int)best.WX; T.SY = (int)best.SY; T.pitch = (int)best.pitch; T.LY = (int)best.LY; T.NPL = (int)best.NPL; T.LYA = (int)best.LYA;
  T.nblocks = (int)best.nb; T.segs = (int)best.segs; T.seglen = (int)best.seglen;
  T.n_cols = (int)A.n_cols; T.ncls = (int)ncls;
  T.oxl = T.oyl = T.ozl = 0; T.oxh = (int)n1; T.oyh = (int)n2; T.ozh = (int)n3;   // ||r||^2 over every row (mg_ghost_*: the owned box, set per launch)
  A.rm4 = T;
  A.rm4_lds = best.lds;
  A.rm4_k1 = (int)best.K1;
  A.rm4_nt = (int)best.NT;
  A.rm4_fill = best.fill;
  A.rc_march4 = true;
  if (A.opt.debug_format)
    std::fprintf(stderr, "[mg] march4: tiles %lldx%lld of %lldx%lld (%lld threads, K1 %lld, SY %lld), %lld segments of %lld planes, LDS %zu B, est. %.1f B/row\n",
                 best.tilesx, best.tilesy, best.TX, best.TY, best.NT, best.K1, best.SY, best.segs, best.seglen, best.lds, best.fill);
  return MG_OK;
}

// Class ids as a product of three index maps, cls(x, y, z) = tab[cz[z]][cy[y]][cx[x]] (hash of every x-slice / y-slice /
// z-slice of the class array; equal hashes = same index; then the exact check, row by row), every entry of every class
// inside the grid wherever the class occurs.  cmap = cx[n1] | cy[n2] | cz[n3] | tab.  false: not such an operator.
static bool class_product_map(const unsigned short* cl, long long n1, long long n2, long long n3, size_t ncls,
                              const std::vector<std::vector<M3Ent>>& ents, bool box, std::vector<unsigned short>& cmap,
                              int& ncx, int& ncy, int& ncz) {
  using Ent = M3Ent;
  cmap.clear();
  std::vector<unsigned long long> hx((size_t)n1, 0), hy((size_t)n2, 0), hz((size_t)n3, 0);
  auto mix = [](unsigned long long v) {
    v ^= v >> 33; v *= 0xff51afd7ed558ccdULL; v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ULL; v ^= v >> 33;
    return v;
  };
  for (long long z = 0; z < n3; ++z)
    for (long long y = 0; y < n2; ++y) {
      const unsigned short* line = cl + (z * n2 + y) * n1;
      unsigned long long hl = 0;
      for (long long x = 0; x < n1; ++x) {
        const unsigned long long v = (unsigned long long)line[x] + 1;
        hx[(size_t)x] += mix(v * 0x9E3779B97F4A7C15ULL + (unsigned long long)(z * n2 + y));
        hl += mix(v * 0xD6E8FEB86659FD93ULL + (unsigned long long)x);
      }
      hy[(size_t)y] += mix(hl + (unsigned long long)z * 0x9E3779B97F4A7C15ULL);
      hz[(size_t)z] += mix(hl + (unsigned long long)y * 0xC2B2AE3D27D4EB4FULL);
    }
  auto index_of = [](const std::vector<unsigned long long>& hv, std::vector<unsigned short>& idx, std::vector<long long>& rep) {
    std::unordered_map<unsigned long long, int> seen;
    idx.resize(hv.size());
    for (size_t i = 0; i < hv.size(); ++i) {
      auto itf = seen.find(hv[i]);
      if (itf == seen.end()) {
        itf = seen.emplace(hv[i], (int)rep.size()).first;
        rep.push_back((long long)i);
      }
      idx[i] = (unsigned short)itf->second;
    }
  };
  std::vector<unsigned short> cx, cy, cz;
  std::vector<long long> rx, ry, rz;
  index_of(hx, cx, rx);
  index_of(hy, cy, ry);
  index_of(hz, cz, rz);
  ncx = (int)rx.size(); ncy = (int)ry.size(); ncz = (int)rz.size();
  if ((long long)ncx * ncy * ncz > mgk::RM3_TAB) return false;
  std::vector<unsigned short> tab((size_t)ncx * ncy * ncz);
  for (int iz = 0; iz < ncz; ++iz)
    for (int iy = 0; iy < ncy; ++iy)
      for (int ix = 0; ix < ncx; ++ix) tab[((size_t)iz * ncy + iy) * ncx + ix] = cl[(rz[(size_t)iz] * n2 + ry[(size_t)iy]) * n1 + rx[(size_t)ix]];
  bool okmap = true;
#pragma omp parallel for schedule(static) reduction(&& : okmap)
  for (long long z = 0; z < n3; ++z) {
    for (long long y = 0; y < n2 && okmap; ++y) {
      const unsigned short* line = cl + (z * n2 + y) * n1;
      const unsigned short* trow = tab.data() + ((size_t)cz[(size_t)z] * ncy + cy[(size_t)y]) * ncx;
      for (long long x = 0; x < n1; ++x)
        if (line[x] != trow[cx[(size_t)x]]) { okmap = false; break; }
    }
  }
  if (!okmap) return false;     // the classes are not a product of coordinate classes: the 1-D chunk form serves the level
  for (unsigned short v : tab) if (v >= ncls && !(box && v == 0xFFFF)) return false;
  // Every entry of every class must point INSIDE the grid wherever the class occurs: the tile kernels read the in-plane
  // neighbours of stage 2 (and later) from slabs that hold computed rows only - a wrap-around coupling (periodic in x: the
  // shift n1 - 1 decomposes as dy = +1, dx = -1 and passes every check above) would read a line outside the grid as zeros.
  // Such operators keep the 1-D chunk form / two launches, whose linear indexing computes them correctly.
  {
    auto span = [](const std::vector<unsigned short>& idx, int nidx, std::vector<long long>& lo, std::vector<long long>& hi) {
      lo.assign((size_t)nidx, (long long)idx.size());
      hi.assign((size_t)nidx, -1);
      for (size_t i = 0; i < idx.size(); ++i) {
        lo[idx[i]] = std::min<long long>(lo[idx[i]], (long long)i);
        hi[idx[i]] = std::max<long long>(hi[idx[i]], (long long)i);
      }
    };
    std::vector<long long> xlo, xhi, ylo, yhi, zlo, zhi;
    span(cx, ncx, xlo, xhi);
    span(cy, ncy, ylo, yhi);
    span(cz, ncz, zlo, zhi);
    for (int iz = 0; iz < ncz; ++iz)
      for (int iy = 0; iy < ncy; ++iy)
        for (int ix = 0; ix < ncx; ++ix) {
          const unsigned short c = tab[((size_t)iz * ncy + iy) * ncx + ix];
          if (c == 0xFFFF) continue;
          for (const Ent& t : ents[c])
            if (xlo[(size_t)ix] + t.dx < 0 || xhi[(size_t)ix] + t.dx >= n1 || ylo[(size_t)iy] + t.dy < 0 || yhi[(size_t)iy] + t.dy >= n2 ||
                zlo[(size_t)iz] + t.dz < 0 || zhi[(size_t)iz] + t.dz >= n3)
              return false;
        }
  }
  cmap.insert(cmap.end(), cx.begin(), cx.end());
  cmap.insert(cmap.end(), cy.begin(), cy.end());
  cmap.insert(cmap.end(), cz.begin(), cz.end());
  cmap.insert(cmap.end(), tab.begin(), tab.end());
  return true;
}

int build_march3_impl(Csr& A, const long long grid[3], const unsigned short* cl_in, size_t ncls,
                      const std::vector<std::vector<M3Ent>>& ents, bool var, bool canon) {
  using Ent = M3Ent;
  const bool box = A.regular_cols >= 0;
  const long long nreg = box ? A.regular_cols : A.n_rows;
  const long long n1 = grid[0], n2 = grid[1], n3 = grid[2];
  const long long P = n1 * n2;
  // ---- class ids as a product of three index maps --------------------------------------------------------------------------
  std::vector<unsigned short> cmap;
  int ncx = 0, ncy = 0, ncz = 0;
  {
    if (!class_product_map(cl_in, n1, n2, n3, ncls, ents, box, cmap, ncx, ncy, ncz)) return MG_OK;
    const unsigned short* cl = cl_in;
    if (box && A.rc_nexc > 0) {
      // Stage 2 (r = b - A t) of a row next to an exception row needs that row's t, which exists only after the exchange:
      // such rows (the layer behind the faces) are left to csr_rows_spmv as well.  Their set must be sx[x] | sy[y] | sz[z].
      std::vector<unsigned char> near((size_t)nreg, 0);
#pragma omp parallel for schedule(static)
      for (long long i = 0; i < nreg; ++i) {
        const unsigned short c = cl[i];
        if (c == 0xFFFF) continue;
        for (int k = A.h_rc_ptr[c]; k < A.h_rc_ptr[(size_t)c + 1]; ++k) {
          const long long col = i + A.h_rc_delta[c] + A.h_rc_off[(size_t)k];
          if (col >= 0 && col < nreg && cl[col] == 0xFFFF) { near[(size_t)i] = 1; break; }
        }
      }
      std::vector<unsigned short> sx((size_t)n1, 1), sy((size_t)n2, 1), sz((size_t)n3, 1);
      for (long long z = 0; z < n3; ++z)
        for (long long y = 0; y < n2; ++y)
          for (long long x = 0; x < n1; ++x) {
            const long long i = (z * n2 + y) * n1 + x;
            if (cl[i] == 0xFFFF || near[(size_t)i]) continue;
            sx[(size_t)x] = 0; sy[(size_t)y] = 0; sz[(size_t)z] = 0;     // a row computed in full: none of its coordinates is flagged
          }
      std::vector<int> list2;
      for (long long z = 0; z < n3; ++z)
        for (long long y = 0; y < n2; ++y)
          for (long long x = 0; x < n1; ++x) {
            const long long i = (z * n2 + y) * n1 + x;
            if (cl[i] == 0xFFFF) continue;
            const bool flag = sx[(size_t)x] | sy[(size_t)y] | sz[(size_t)z];
            if (near[(size_t)i] && !flag) return MG_OK;                 // not a union of coordinate layers: two launches per pair
            if (flag) list2.push_back((int)i);                          // (a superset of `near` is harmless: computed by the list kernel)
          }
      cmap.insert(cmap.end(), sx.begin(), sx.end());
      cmap.insert(cmap.end(), sy.begin(), sy.end());
      cmap.insert(cmap.end(), sz.begin(), sz.end());
      A.rc_nexc2 = (int)list2.size();
      if (!list2.empty()) {
        MG_TRY(A.rc_exc2.alloc(list2.size()));
        HIP_TRY(hipMemcpy(A.rc_exc2.p, list2.data(), list2.size() * sizeof(int), hipMemcpyHostToDevice));
      }
    }
  }
  // ---- tile geometry ------------------------------------------------------------------------------------------------------
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const long long lds_cap = 160 * 1024 - 1024;
  const size_t dict_bytes = ncls * (sizeof(mgk::M3Class) + 8) + ((cmap.size() * 2 + 15) & ~(size_t)15);
  struct Geo { long long NT, tilesx, TX, TY, tilesy, WX, SY, NPL, pitch, LY, K1, nb, segs, seglen; size_t lds; double fill; };
  Geo best{};
  bool have = false;
  // (VAR: 3 x 8 more doubles per row and lane in registers - 512 threads, 256 registers per lane, two or three rows per lane)
  for (long long NT : {1024LL, 768LL, 512LL}) {
    if (var != (NT == 512)) continue;
    if (!var && A.opt.march3_nt != 0 && A.opt.march3_nt != NT) continue;
    for (long long K1 = 2; K1 <= (NT == 768 ? 4 : 3); ++K1) {
      if (A.opt.march3_k1 != 0 && K1 != A.opt.march3_k1 && !(var && A.opt.march3_k1 > 3)) continue;
      if (NT == 768 && K1 < 3) continue;
      for (long long tilesx = 1; tilesx <= std::max<long long>({1, n1 / 16, A.opt.march3_tiles_x}); ++tilesx) {
        if (A.opt.march3_tiles_x > 0 && tilesx != A.opt.march3_tiles_x) continue;
        Geo g{};
        g.NT = NT;
        g.K1 = K1;
        g.tilesx = tilesx;
        g.TX = (n1 + tilesx - 1) / tilesx;
        g.WX = g.TX + 2;
        if (g.WX > NT / 2) continue;
        g.SY = NT / g.WX;
        g.TY = std::min<long long>(K1 * g.SY - 2, n2);
        if (g.TY < 2) continue;
        g.tilesy = (n2 + g.TY - 1) / g.TY;
        g.TY = (n2 + g.tilesy - 1) / g.tilesy;                        // equal tiles
        g.NPL = (g.TX + 6) / 2;
        g.pitch = 2 * g.NPL;
        g.LY = g.TY + 4;
        if (g.LY * g.NPL > (long long)RM3_NPM * NT) continue;
        g.lds = (size_t)(3 * g.LY + 2 * (g.TY + 2)) * (size_t)g.pitch * 8 + dict_bytes;
        if ((long long)g.lds > lds_cap) continue;
        const long long wg_per_cu = 1;   // (> 100 registers per lane: one workgroup of 12-16 waves per CU whatever the LDS)
        const long long tiles = g.tilesx * g.tilesy, items = tiles * n3, slots = wg_per_cu * ncu;
        // balanced: equal contiguous ranges of the (tile, plane) list; lockstep: tiles x segments
        g.nb = std::max<long long>(1, std::min<long long>(slots, items / 4));
        double R = (double)items / (double)g.nb, eff = 1.0;
        g.segs = 0;
        g.seglen = 0;
        if (!A.opt.no_march3_lockstep && tiles <= slots) {
          const long long S = std::min<long long>(slots / tiles, n3 / 4);
          if (S >= 1) {
            const long long Lz = (n3 + S - 1) / S;
            const double e = ((double)n3 / (double)(S * Lz)) * ((double)(tiles * S) / (double)slots);
            if (e >= 0.85 || A.opt.march3_lockstep_force) {
              g.segs = S;
              g.seglen = Lz;
              g.nb = tiles * S;
              R = (double)Lz;
              eff = e;
            }
          }
        }
        const double core = (double)g.TX * (double)g.TY;
        // fills per row of the grid: tiles are equal, so partial tiles at the far edges are charged through tiles*core / P;
        // a line segment of W doubles at an arbitrary alignment touches W/16 + 15/16 cache lines of 128 bytes
        const double waste = (double)(g.tilesx * g.TX) * (double)(g.tilesy * g.TY) / (double)P;
        auto lines = [](double W) { return 1.0 + 15.0 / W; };
        // (lockstep: neighbouring tiles stage their common halo lines at the same time on one XCD - measured on 257^3: the
        // fabric traffic falls to 1.02 x compulsory, the pass gains 5 %: the halo excess is charged at half)
        const double share = g.segs > 0 ? 0.5 : 1.0;
        const double fx = 8.0 * (double)((g.TX + 4) * (g.TY + 4)) / core * (1.0 + 3.0 / R) * lines((double)(g.TX + 4));
        const double fb = 8.0 * (double)((g.TX + 2) * (g.TY + 2)) / core * (1.0 + 2.0 / R) * lines((double)(g.TX + 2));
        g.fill = (waste * (8.0 + share * (fx - 8.0) + 8.0 + share * (fb - 8.0)) + 16.0) / eff;
        if (!have || g.fill < best.fill) {
          best = g;
          have = true;
        }
      }
    }
  }
  if (!have) return MG_OK;
  if (best.nb < std::min<long long>(A.opt.march_min_wg, (long long)ncu * 3 / 4)) return MG_OK;   // small levels: latency-bound, other kernels
  // ---- class records with byte offsets in the chosen pitch ------------------------------------------------------------------
  std::vector<mgk::M3Class> recs(ncls);
  for (size_t c = 0; c < ncls; ++c) {
    mgk::M3Class q{};
    int nip = 0, first_off = 0;
    std::vector<double> vals(ents[c].size(), 1.0);   // (VAR: the records carry the structure only)
    if (!var) {
      const int k0 = A.h_rc_ptr[c];
      vals.resize((size_t)(A.h_rc_ptr[c + 1] - k0));
      if (!vals.empty()) HIP_TRY(hipMemcpy(vals.data(), A.rc_val.p + k0, vals.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (size_t e = 0; e < ents[c].size(); ++e) {
      const Ent& t = ents[c][e];
      if (t.dz == -1) q.v_lo = vals[e];
      else if (t.dz == 1) q.v_hi = vals[e];
      else {
        const int off = (int)((t.dy * best.pitch + t.dx) * 8);
        if (nip == 0) first_off = off;
        q.v[nip] = vals[e];
        q.off[nip] = off;
        ++nip;
      }
    }
    for (int u = nip; u < mgk::RM3_NIP; ++u) {
      q.v[u] = 0.0;
      q.off[u] = first_off;
    }
    if (var && canon) {     // band form in canonical slots: the five in-plane offsets of the star, whatever the class holds (value 0 where it has none)
      const int co[5] = {-(int)best.pitch * 8, -8, 0, 8, (int)best.pitch * 8};
      for (int u = 0; u < 5 && u < mgk::RM3_NIP; ++u) { q.v[u] = 1.0; q.off[u] = co[u]; }
    }
    q.flags = 0;
    recs[c] = q;
  }
  MG_TRY(A.rm3_cls.alloc(ncls));
  HIP_TRY(hipMemcpy(A.rm3_cls.p, recs.data(), ncls * sizeof(mgk::M3Class), hipMemcpyHostToDevice));
  MG_TRY(A.rm3_cmap.alloc(cmap.size()));
  HIP_TRY(hipMemcpy(A.rm3_cmap.p, cmap.data(), cmap.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  mgk::March3Dev T{};
  T.cls = A.rm3_cls.p;
  T.cmap = A.rm3_cmap.p;
  T.ncx = ncx; T.ncy = ncy; T.ntab = ncx * ncy * ncz;
  T.n1 = (int)n1; T.n2 = (int)n2; T.nplanes = (int)n3; T.P = (int)P;
  T.TX = (int)best.TX; T.TY = (int)best.TY; T.tiles_x = (int)best.tilesx; T.tiles_y = (int)best.tilesy;
  T.WX = (int)best.WX; T.SY = (int)best.SY; T.pitch = (int)best.pitch; T.LY = (int)best.LY; T.NPL = (int)best.NPL;
  T.nblocks = (int)best.nb;
  T.segs = (int)best.segs; T.seglen = (int)best.seglen;
  T.n_cols = (int)A.n_cols; T.ncls = (int)ncls;
  T.has_exc = (box && A.rc_nexc > 0) ? 1 : 0;
  A.rm3 = T;
  A.rm3_lds = best.lds;
  A.rm3_k1 = (int)best.K1;
  A.rm3_nt = (int)best.NT;
  A.rm3_fill = best.fill;
  A.rc_march3 = true;
  if (!var && !box) MG_TRY(build_march4(A, recs, ents, ncx, ncy, ncz, (cmap.size() * 2 + 15) & ~(size_t)15, ncu, cmap.data() + n1));
  if (A.opt.debug_format)
    std::fprintf(stderr, "[mg] march3: grid %lldx%lldx%lld tiles %lldx%lld of %lldx%lld (%lld threads, K1 %lld, SY %lld), %lld workgroups%s, class maps %dx%dx%d, LDS %zu B, est. %.1f B/row\n",
                 n1, n2, n3, best.tilesx, best.tilesy, best.TX, best.TY, best.NT, best.K1, best.SY, best.nb,
                 best.segs ? " (lockstep)" : "", ncx, ncy, ncz, best.lds, best.fill);
  return MG_OK;
}

// 27-point form (csr_rowclass_march27_spmv): a square grid operator in row-class form (implicit first column, no exception
// rows, relaxPrec per class) that the z-star tile forms do not serve, every entry a shift (dz, dy, dx) in {-1, 0, 1}^3 in
// ascending order, classes a verified product map.  Two geometries: [0] one product per walk (region = core), [1] sweep +
// residual (stage 1 on core + one ring, 4 + 4 slabs).  Workgroups = tiles x segments of planes, several rounds of the CUs
// allowed; cost = rounds x (planes per segment + run-in + ring fill) x time per iteration (grows with lanes x rows per lane).
int build_march27(Csr& A, const long long grid[3]) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  A.rc_march27 = false;
  if (A.opt.no_march27 || A.opt.no_march || A.rc_march3) return MG_OK;
  if (!A.has_rc || !A.rc_implicit || A.h_rc_ptr.empty() || A.rc_nexc != 0 || A.regular_cols >= 0 || !A.rc_has_d || A.n_rows != A.n_cols) return MG_OK;
  const long long n1 = grid[0], n2 = grid[1], n3 = grid[2];
  if (n1 < 8 || n2 < 8 || n3 < 8 || n1 * n2 * n3 != A.n_rows || A.n_rows < A.opt.march27_min_rows) return MG_OK;
  if (n1 > 65535 || n2 > 65535 || n3 > 65535 || A.h_cls.size() != (size_t)A.n_rows) return MG_OK;
  const long long P = n1 * n2;
  if (A.n_rows + 8 * P >= (1LL << 31) - 1) return MG_OK;   // int32 row arithmetic in the kernel
  const size_t ncls = A.h_rc_ptr.size() - 1;
  if (ncls > 64 || (size_t)A.rc_ncls != ncls) return MG_OK;
  std::vector<std::vector<M3Ent>> ents(ncls);
  std::vector<mgk::M27Class> recs(ncls);
  std::vector<double> dcls(ncls);
  HIP_TRY(hipMemcpy(dcls.data(), A.rc_d.p, ncls * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t c = 0; c < ncls; ++c) {
    const int k0 = A.h_rc_ptr[c], k1 = A.h_rc_ptr[c + 1];
    std::vector<double> vals((size_t)(k1 - k0));
    if (!vals.empty()) HIP_TRY(hipMemcpy(vals.data(), A.rc_val.p + k0, vals.size() * sizeof(double), hipMemcpyDeviceToHost));
    mgk::M27Class q{};
    q.d = dcls[c];
    int last = -1;
    for (int k = k0; k < k1; ++k) {
      const long long sh = (long long)A.h_rc_delta[c] + A.h_rc_off[(size_t)k];
      const long long dz = (sh >= 0) ? (sh + P / 2) / P : -((-sh + P / 2) / P);
      const long long rest = sh - dz * P;
      const long long dy = (rest >= 0) ? (rest + n1 / 2) / n1 : -((-rest + n1 / 2) / n1);
      const long long dx = rest - dy * n1;
      if (dz < -1 || dz > 1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) return MG_OK;
      const int slot = (int)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
      if (slot <= last) return MG_OK;                               // (ascending columns: the order of the products)
      last = slot;
      q.v[slot] = vals[(size_t)(k - k0)];
      ents[c].push_back({(int)dz, (int)dy, (int)dx});
    }
    recs[c] = q;
  }
  std::vector<unsigned short> cmap;
  int ncx = 0, ncy = 0, ncz = 0;
  if (!class_product_map(A.h_cls.data(), n1, n2, n3, ncls, ents, false, cmap, ncx, ncy, ncz)) return MG_OK;
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const long long lds_cap = 160 * 1024 - 1024;
  const size_t dict_bytes = ncls * sizeof(mgk::M27Class) + ((((size_t)n3 + (size_t)ncx * ncy * ncz) * 2 + 15) & ~(size_t)15);
  struct Geo { long long NT, tilesx, TX, TY, tilesy, WX, SY, NPL, pitch, LY, nb, segs, seglen; size_t lds; double cost; };
  Geo best[2]{};
  for (int two = 0; two < 2; ++two) {
    bool have = false;
    const long long G1 = two ? 1 : 0, NSL = two ? 4 : 2, RI = two ? 5 : 2;   // (run-in: iterations of a segment beyond its planes)
    for (long long NT : {1024LL, 512LL, 256LL}) {
      if (A.opt.march27_nt != 0 && A.opt.march27_nt != NT) continue;
      for (long long tilesx = 1; tilesx <= std::max<long long>({1, n1 / 8, A.opt.march27_tiles_x}); ++tilesx) {
        if (A.opt.march27_tiles_x > 0 && tilesx != A.opt.march27_tiles_x) continue;
        Geo g{};
        g.NT = NT; g.tilesx = tilesx;
        g.TX = (n1 + tilesx - 1) / tilesx;
        g.WX = g.TX + 2 * G1;
        if (g.WX > NT / 4) continue;
        g.NPL = (g.WX + 4) / 2;
        g.pitch = 0;
        for (long long pt : {24LL, 32LL, 40LL, 48LL, 64LL})        // (the instantiated pitches)
          if (g.pitch == 0 && pt >= 2 * g.NPL) g.pitch = pt;
        if (g.pitch == 0) continue;
        auto fits = [&](long long ty) {
          const long long ly = ty + 2 * G1 + 2;
          return ty >= 2 && ly * g.NPL <= NT && (long long)((size_t)NSL * (size_t)ly * (size_t)g.pitch * 8 + dict_bytes) <= lds_cap;
        };
        long long TY = std::min<long long>(NT / g.WX - 2 * G1, n2);   // one row per lane: the region's lines
        while (TY >= 2 && !fits(TY)) --TY;
        if (TY < 2) continue;
        g.tilesy = (n2 + TY - 1) / TY;
        g.TY = (n2 + g.tilesy - 1) / g.tilesy;                      // equal tiles
        g.SY = g.TY + 2 * G1;
        g.LY = g.SY + 2;
        g.lds = (size_t)NSL * (size_t)g.LY * (size_t)g.pitch * 8 + dict_bytes;
        // workgroups a CU holds side by side: 16 wavefronts (<= 128 registers per lane) and the LDS; several small workgroups
        // hide one another's load latency (an iteration of this kernel is shorter than a trip to memory), at the price of more halo
        long long wpc = std::min<long long>(1024 / NT, (160 * 1024) / (long long)g.lds);
        if (A.opt.march27_wgs > 0) wpc = std::min<long long>(wpc, A.opt.march27_wgs);
        if (wpc < 1) continue;
        const long long tiles = g.tilesx * g.tilesy, slots = ncu * wpc;
        long long S = 1, rounds = (tiles + slots - 1) / slots;
        double bestr = 0.0;
        for (long long sc = 1; sc <= std::max<long long>(1, n3 / 4); ++sc) {
          if (A.opt.march27_segs > 0 && sc != A.opt.march27_segs) continue;
          const long long lz = (n3 + sc - 1) / sc, rd = (tiles * sc + slots - 1) / slots;
          const double cst = (double)rd * (double)(lz + RI + 1);
          if (bestr == 0.0 || cst < bestr) { bestr = cst; S = sc; rounds = rd; }
        }
        const long long Lz = (n3 + S - 1) / S;
        g.segs = S; g.seglen = Lz; g.nb = tiles * S;
        // time per iteration of a CU's workgroups: the work of wpc x NT rows, or the trip to memory an iteration waits for when a
        // workgroup runs alone (fit to profiles/r04_march27_ab.md)
        const double work = (two ? 0.55e-3 : 0.3e-3) * (double)(NT * wpc) + 0.15 * (double)wpc;
        g.cost = (double)rounds * (double)(Lz + RI + 1) * std::max(work, 1.5 / (double)wpc + 0.2);
        if (!have || g.cost < best[two].cost) {
          best[two] = g;
          have = true;
        }
      }
    }
    if (!have) return MG_OK;
  }
  MG_TRY(A.rm27_cls.alloc(ncls));
  HIP_TRY(hipMemcpy(A.rm27_cls.p, recs.data(), ncls * sizeof(mgk::M27Class), hipMemcpyHostToDevice));
  MG_TRY(A.rm27_cmap.alloc(cmap.size()));
  HIP_TRY(hipMemcpy(A.rm27_cmap.p, cmap.data(), cmap.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  if (A.rm27_sink.n < (size_t)8 * 32 * 1024) {
    MG_TRY(A.rm27_sink.alloc((size_t)8 * 32 * 1024));
    HIP_TRY(hipMemset(A.rm27_sink.p, 0, A.rm27_sink.bytes()));
  }
  for (int two = 0; two < 2; ++two) {
    const Geo& g = best[two];
    mgk::March27Dev T{};
    T.cls = A.rm27_cls.p;
    T.cmap = A.rm27_cmap.p;
    T.ncx = ncx; T.ncy = ncy; T.ncz = ncz; T.ntab = ncx * ncy * ncz;
    T.n1 = (int)n1; T.n2 = (int)n2; T.nplanes = (int)n3; T.P = (int)P;
    T.TX = (int)g.TX; T.TY = (int)g.TY; T.tiles_x = (int)g.tilesx; T.tiles_y = (int)g.tilesy;
    T.WX = (int)g.WX; T.SY = (int)g.SY; T.LY = (int)g.LY; T.NPL = (int)g.NPL;
    T.nblocks = (int)g.nb; T.segs = (int)g.segs; T.seglen = (int)g.seglen;
    T.n_cols = (int)A.n_cols; T.ncls = (int)ncls;
    A.rm27[two] = T;
    A.rm27_lds[two] = g.lds;
    A.rm27_nt[two] = (int)g.NT;
    A.rm27_pitch[two] = (int)g.pitch;
    if (A.opt.debug_format)
      std::fprintf(stderr, "[mg] march27 (%s): grid %lldx%lldx%lld tiles %lldx%lld of %lldx%lld (%lld threads, region %lldx%lld, pitch %lld), %lld segments of %lld planes = %lld workgroups, LDS %zu B\n",
                   two ? "pair" : "single", n1, n2, n3, g.tilesx, g.tilesy, g.TX, g.TY, g.NT, g.WX, g.SY, g.pitch, g.segs, g.seglen, g.nb, g.lds);
  }
  A.rc_march27 = true;
  return MG_OK;
}

// Marching restriction (csr_rowclass_marchr_spmv): R in row-class form with explicit first columns, no exception rows, rows = a
// coarse grid gc, columns = a fine grid gf with gf = 2*gc - 1 per direction; every entry of every row must be a fine node
// (2i + dx, 2j + dy, 2k + dz), |d| <= 1, in ascending order - derived per class from one row and VERIFIED on every row (first
// column against the row's centre), classes a verified product map over the coarse grid.  Geometry: TX x TY coarse columns per
// workgroup (one per lane), segments of coarse planes; several workgroups per CU.
int build_marchr(Csr& R, const long long gf[3], const long long gc[3]) {
  if (R.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  R.rc_marchr = false;
  if (R.opt.no_marchr || R.opt.no_march || !R.has_rc || R.rc_implicit || R.h_rc_ptr.empty() || R.rc_nexc != 0 || R.regular_cols >= 0) return MG_OK;
  const long long nc1 = gc[0], nc2 = gc[1], nc3 = gc[2], nf1 = gf[0], nf2 = gf[1], nf3 = gf[2];
  if (nc1 < 4 || nc2 < 4 || nc3 < 4 || nf1 != 2 * nc1 - 1 || nf2 != 2 * nc2 - 1 || nf3 != 2 * nc3 - 1) return MG_OK;
  if (nc1 * nc2 * nc3 != R.n_rows || nf1 * nf2 * nf3 != R.n_cols || R.n_rows < R.opt.marchr_min_rows) return MG_OK;
  if (R.n_cols + 4 * nf1 * nf2 >= (1LL << 31) - 1 || nc1 > 65535 || nc2 > 65535 || nc3 > 65535) return MG_OK;
  if (R.h_cls.size() != (size_t)R.n_rows || R.h_rp.size() != (size_t)R.n_rows + 1) return MG_OK;
  const size_t ncls = R.h_rc_ptr.size() - 1;
  if (ncls > 64 || (size_t)R.rc_ncls != ncls) return MG_OK;
  const long long Pf = nf1 * nf2, Pc = nc1 * nc2;
  auto centre = [&](long long row) {
    const long long k = row / Pc, rem = row - k * Pc, jy = rem / nc1, ix = rem - jy * nc1;
    return (2 * k) * Pf + (2 * jy) * nf1 + 2 * ix;
  };
  // per class: the shift of the first column against the centre, from the first row of the class
  std::vector<long long> s0(ncls, LLONG_MIN);
  for (long long i = 0; i < R.n_rows; ++i) {
    const unsigned short c = R.h_cls[(size_t)i];
    if (c >= ncls) return MG_OK;
    if (R.h_rp[(size_t)i + 1] == R.h_rp[(size_t)i]) return MG_OK;
    const long long sh = (long long)R.h_ci[(size_t)R.h_rp[(size_t)i]] - centre(i);
    if (s0[c] == LLONG_MIN) s0[c] = sh;
    else if (s0[c] != sh) return MG_OK;                             // rows of one class whose entries sit differently around their centres
  }
  std::vector<std::vector<M3Ent>> ents(ncls);
  std::vector<mgk::M27Class> recs(ncls);
  for (size_t c = 0; c < ncls; ++c) {
    if (s0[c] == LLONG_MIN) continue;                               // (a class no row has)
    const int k0 = R.h_rc_ptr[c], k1 = R.h_rc_ptr[c + 1];
    std::vector<double> vals((size_t)(k1 - k0));
    if (!vals.empty()) HIP_TRY(hipMemcpy(vals.data(), R.rc_val.p + k0, vals.size() * sizeof(double), hipMemcpyDeviceToHost));
    mgk::M27Class q{};
    int last = -1;
    for (int k = k0; k < k1; ++k) {
      const long long sh = s0[c] + (long long)R.h_rc_off[(size_t)k];
      const long long dz = (sh >= 0) ? (sh + Pf / 2) / Pf : -((-sh + Pf / 2) / Pf);
      const long long rest = sh - dz * Pf;
      const long long dy = (rest >= 0) ? (rest + nf1 / 2) / nf1 : -((-rest + nf1 / 2) / nf1);
      const long long dx = rest - dy * nf1;
      if (dz < -1 || dz > 1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) return MG_OK;
      const int slot = (int)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
      if (slot <= last) return MG_OK;
      last = slot;
      q.v[slot] = vals[(size_t)(k - k0)];
      ents[c].push_back({(int)dz, (int)dy, (int)dx});
    }
    recs[c] = q;
  }
  std::vector<unsigned short> cmap;
  int ncx = 0, ncy = 0, ncz = 0;
  if (!class_product_map(R.h_cls.data(), nc1, nc2, nc3, ncls, ents, false, cmap, ncx, ncy, ncz)) return MG_OK;
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  // 256 threads: 32 x 8 coarse columns over a 65 x 17 fine slab (pitch 72, three pairs per lane), four workgroups per CU
  const long long NT = 256, TX = R.opt.marchr_tx > 0 ? R.opt.marchr_tx : 32, TY = R.opt.marchr_ty > 0 ? R.opt.marchr_ty : NT / TX;
  if (TX * TY > NT || TX < 2 || TY < 1) return MG_OK;
  const long long NPL = TX + 2, pitch = 72, LY = 2 * TY + 1;
  if (2 * NPL > pitch || LY * NPL > 3 * NT) return MG_OK;
  const size_t dict_bytes = ncls * sizeof(mgk::M27Class) + ((((size_t)nc3 + (size_t)ncx * ncy * ncz) * 2 + 15) & ~(size_t)15);
  const size_t lds = (size_t)2 * (size_t)LY * (size_t)pitch * 8 + dict_bytes;
  if (lds > 60 * 1024) return MG_OK;   // (below the 64 KB a launch gets without the function attribute)
  const long long tilesx = (nc1 + TX - 1) / TX, tilesy = (nc2 + TY - 1) / TY, tiles = tilesx * tilesy, slots = 4LL * ncu;
  long long S = 1;
  {
    double bestr = 0.0;
    for (long long sc = 1; sc <= std::max<long long>(1, nc3 / 4); ++sc) {
      if (R.opt.marchr_segs > 0 && sc != R.opt.marchr_segs) continue;
      const long long lz = (nc3 + sc - 1) / sc, rd = (tiles * sc + slots - 1) / slots;
      const double cst = (double)rd * (double)(2 * lz + 1 + 12);     // (fine planes of a segment + the launch's ramp, in iterations)
      if (bestr == 0.0 || cst < bestr) { bestr = cst; S = sc; }
    }
  }
  MG_TRY(R.rmr_cls.alloc(ncls));
  HIP_TRY(hipMemcpy(R.rmr_cls.p, recs.data(), ncls * sizeof(mgk::M27Class), hipMemcpyHostToDevice));
  MG_TRY(R.rmr_cmap.alloc(cmap.size()));
  HIP_TRY(hipMemcpy(R.rmr_cmap.p, cmap.data(), cmap.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  if (R.rm27_sink.n < (size_t)8 * 32 * 1024) {
    MG_TRY(R.rm27_sink.alloc((size_t)8 * 32 * 1024));
    HIP_TRY(hipMemset(R.rm27_sink.p, 0, R.rm27_sink.bytes()));
  }
  mgk::MarchRDev T{};
  T.cls = R.rmr_cls.p;
  T.cmap = R.rmr_cmap.p;
  T.ncx = ncx; T.ncy = ncy; T.ncz = ncz; T.ntab = ncx * ncy * ncz;
  T.nc1 = (int)nc1; T.nc2 = (int)nc2; T.nc3 = (int)nc3; T.Pc = (int)Pc;
  T.nf1 = (int)nf1; T.nf2 = (int)nf2; T.nf3 = (int)nf3; T.Pf = (int)Pf;
  T.TX = (int)TX; T.TY = (int)TY; T.tiles_x = (int)tilesx; T.tiles_y = (int)tilesy;
  T.LY = (int)LY; T.NPL = (int)NPL;
  T.segs = (int)S; T.seglen = (int)((nc3 + S - 1) / S); T.nblocks = (int)(tiles * S);
  T.n_cols = (int)R.n_cols; T.ncls = (int)ncls;
  R.rmr = T;
  R.rmr_lds = lds;
  R.rc_marchr = true;
  if (R.opt.debug_format)
    std::fprintf(stderr, "[mg] marchr: coarse grid %lldx%lldx%lld tiles %lldx%lld of %lldx%lld, %lld segments of %d planes = %d workgroups, LDS %zu B\n",
                 nc1, nc2, nc3, tilesx, tilesy, TX, TY, S, T.seglen, T.nblocks, lds);
  return MG_OK;
}

// Prolongation-shaped operators (csr_rowclass_winp_spmv): rows = a fine grid gf, columns = a coarse grid gc, explicit
// first columns.  Everything is derived from the stored pattern and checked against it: the coarse plane of each fine
// plane's first columns (cz0), the split of every dictionary offset into plane shift (0 or 1) + in-plane rest, per chunk
// of WP_ROWS in-plane rows the window [wlo, wlo + W) of coarse in-plane indices its rows read in any plane, and per row
// the 16-bit index of its first column inside that window.  Any row that does not fit drops the operator back to the
// lane kernel.
int build_winp(Csr& M, const long long gf[3], const long long gc[3]) {
  if (M.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  if (M.rp_ok && M.rp_PF == gf[0] * gf[1] && M.rp_nplanes == gf[2] && M.rp_PC == gc[0] * gc[1]) return MG_OK;   // (same pattern, same hints)
  M.rp_ok = false;
  // (a prolongation of a sharded level: columns [owned coarse box | halo]; the rows that read the halo are exception rows,
  // computed by csr_rows_spmv behind the exchange - they take no part in the windows)
  const bool boxp = M.regular_cols >= 0;
  if (!M.has_rc || M.rc_implicit || (M.rc_nexc != 0 && !boxp) || M.opt.no_winp || (boxp && M.reg_rows() != M.n_rows)) return MG_OK;
  if (gf[0] < 1 || gf[1] < 1 || gf[2] < 1 || gc[0] < 1 || gc[1] < 1 || gc[2] < 1) return MG_OK;
  if (gf[0] * gf[1] * gf[2] != M.n_rows || gc[0] * gc[1] * gc[2] != (boxp ? M.regular_cols : M.n_cols)) return MG_OK;
  if (M.h_rp.size() != (size_t)M.n_rows + 1 || M.h_cls.size() != (size_t)M.n_rows || M.h_rc_ptr.empty()) return MG_OK;
  if (M.rc_ncls * (long long)M.rc_maxlen > 1024 || M.n_rows < M.opt.winp_min_rows) return MG_OK;   // the padded dictionary lives in LDS (16 KB)
  const long long PF = gf[0] * gf[1], PC = gc[0] * gc[1], nz = gf[2];
  if (PF >= (1LL << 30) || PC < 4) return MG_OK;
  const size_t ncls = M.h_rc_ptr.size() - 1;
  std::vector<long long> rest(M.h_rc_off.size());
  std::vector<int> dzc(M.h_rc_off.size());
  std::vector<long long> cmin(ncls, 0), cmax(ncls, 0);   // per class: smallest / largest in-plane rest, second plane shifted by 0
  std::vector<char> csecond(ncls, 0);
  for (size_t c = 0; c < ncls; ++c)
    for (int k = M.h_rc_ptr[c]; k < M.h_rc_ptr[c + 1]; ++k) {
      const long long off = M.h_rc_off[(size_t)k];
      if (off < 0) return MG_OK;
      const long long d = (off + PC / 2) / PC;
      if (d > 1) return MG_OK;
      dzc[(size_t)k] = (int)d;
      rest[(size_t)k] = off - d * PC;
      cmin[c] = std::min(cmin[c], rest[(size_t)k]);
      cmax[c] = std::max(cmax[c], rest[(size_t)k]);
      if (d) csecond[c] = 1;
    }
  std::vector<int> cz0((size_t)nz, INT_MAX);
  for (long long z = 0; z < nz; ++z)
    for (long long p = 0; p < PF; ++p) {
      const long long i = z * PF + p;
      if (M.h_cls[(size_t)i] == 0xFFFF) continue;                      // (exception row: not served by the windows)
      if (M.h_rp[(size_t)i + 1] == M.h_rp[(size_t)i]) return MG_OK;   // an empty row has no first column
      cz0[(size_t)z] = std::min<long long>(cz0[(size_t)z], M.h_ci[(size_t)M.h_rp[(size_t)i]] / PC);
    }
  for (long long z = 0; z < nz; ++z)
    if (cz0[(size_t)z] == INT_MAX) cz0[(size_t)z] = 0;                 // (a plane of exception rows only)
  const long long chunks = (PF + mgk::WP_ROWS - 1) / mgk::WP_ROWS;
  std::vector<long long> lo((size_t)chunks, LLONG_MAX), hi((size_t)chunks, LLONG_MIN);
  std::vector<char> two((size_t)nz, 0);   // does any row of the plane read the second coarse plane?
  for (long long z = 0; z < nz; ++z)
    for (long long p = 0; p < PF; ++p) {
      const long long i = z * PF + p;
      const unsigned short c = M.h_cls[(size_t)i];
      if (c == 0xFFFF) continue;
      const long long fi = (long long)M.h_ci[(size_t)M.h_rp[(size_t)i]] - (long long)cz0[(size_t)z] * PC;   // in-plane index of the first column
      if (fi < 0 || fi >= PC) return MG_OK;
      if (c >= ncls) return MG_OK;
      if (csecond[c] && (long long)cz0[(size_t)z] + 1 >= gc[2]) return MG_OK;   // would read past the last coarse plane
      if (csecond[c]) two[(size_t)z] = 1;
      const size_t ch = (size_t)(p / mgk::WP_ROWS);
      lo[ch] = std::min(lo[ch], fi + cmin[c]);
      hi[ch] = std::max(hi[ch], fi + cmax[c]);
    }
  long long W = 1;
  for (size_t ch = 0; ch < (size_t)chunks; ++ch) {
    if (lo[ch] == LLONG_MAX) { lo[ch] = 0; hi[ch] = 0; }              // (a chunk of exception rows only)
    W = std::max(W, hi[ch] - lo[ch] + 1);
  }
  W = (W + 1) & ~1LL;   // (the dictionary behind the windows stays 16-byte aligned)
  if (W > 2048) return MG_OK;   // 32 KB of windows per workgroup at most (+ <= 16 KB of dictionary: below the 64 KB default)
  std::vector<unsigned short> wf((size_t)M.n_rows);
  for (long long z = 0; z < nz; ++z)
    for (long long p = 0; p < PF; ++p) {
      const long long i = z * PF + p;
      if (M.h_cls[(size_t)i] == 0xFFFF) { wf[(size_t)i] = 0; continue; }
      const long long fi = (long long)M.h_ci[(size_t)M.h_rp[(size_t)i]] - (long long)cz0[(size_t)z] * PC;
      const long long w = fi - lo[(size_t)(p / mgk::WP_ROWS)];
      if (w < 0 || w >= W) return MG_OK;
      wf[(size_t)i] = (unsigned short)w;
    }
  std::vector<int> code(M.h_rc_off.size()), wlo((size_t)chunks);
  for (size_t k = 0; k < code.size(); ++k) code[k] = (int)(dzc[k] * W + rest[k]);
  for (size_t ch = 0; ch < (size_t)chunks; ++ch) wlo[ch] = (int)lo[ch];
  for (long long z = 0; z < nz; ++z)
    if (!two[(size_t)z]) cz0[(size_t)z] |= 0x40000000;   // one window suffices for this plane
  MG_TRY(M.rp_wf.alloc(wf.size()));
  MG_TRY(M.rp_cz0.alloc(cz0.size()));
  MG_TRY(M.rp_wlo.alloc(wlo.size()));
  MG_TRY(M.rp_code.alloc(code.size()));
  HIP_TRY(hipMemcpy(M.rp_wf.p, wf.data(), wf.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M.rp_cz0.p, cz0.data(), cz0.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M.rp_wlo.p, wlo.data(), wlo.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M.rp_code.p, code.data(), code.size() * sizeof(int), hipMemcpyHostToDevice));
  M.rp_PF = (int)PF;
  M.rp_nplanes = (int)nz;
  M.rp_PC = (int)PC;
  M.rp_W = (int)W;
  M.rp_chunks = (int)chunks;
  M.rp_ok = true;
  if (M.opt.debug_format) std::fprintf(stderr, "[mgvcycle] prolongation-shaped operator %lld x %lld: windows of %lld coarse entries per %d rows\n", M.n_rows, M.n_cols, W, mgk::WP_ROWS);
  return MG_OK;
}

int build_schedule(Csr& M, const long long grid[3], long long nrhs) {
  if (M.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  MG_TRY(build_schedule_for(M, grid, nrhs, M.h_blk_row, M.nblocks, M.sched, M.has_sched));
  M.ln_rows = M.ln_blocks = 0;
  M.has_sched_ln = false;
  if (nrhs > 1 && M.set && M.rc_lane_mm()) {   // uniform row blocks of the lane SpMM for this nrhs
    M.ln_rows = lane_mm_rpl(M, nrhs) * (mgk::BLK / lane_mm_group(M, nrhs));
    M.ln_blocks = (int)((M.n_rows + M.ln_rows - 1) / M.ln_rows);
    std::vector<int> blk((size_t)M.ln_blocks + 1);
    for (int b = 0; b <= M.ln_blocks; ++b) blk[(size_t)b] = (int)std::min<long long>((long long)b * M.ln_rows, M.n_rows);
    MG_TRY(build_schedule_for(M, grid, nrhs, blk, M.ln_blocks, M.sched_ln, M.has_sched_ln));
  }
  return build_schedule_for(M, grid, nrhs, M.h_blk_row_mm, M.nblocks_mm, M.sched_mm, M.has_sched_mm);
}
int build_schedule_for(Csr& M, const long long grid[3], long long nrhs, const std::vector<int>& h_blk, int nb,
                       DevBuf<int>& sched, bool& has) {
  has = false;
  if (!M.set || grid[0] <= 0) return MG_OK;
  const long long n1 = grid[0], n2 = grid[1], n3 = std::max<long long>(1, grid[2]);
  if (n1 * n2 * n3 != M.n_rows || n3 < 2 || n2 < 8) return MG_OK;
  // gathered-vector bytes per (y,z) line of the row grid, three z-planes in the window
  const double line_bytes = 3.0 * ((double)M.n_cols / (double)(n2 * n3)) * 8.0 * (double)nrhs;
  const double plane_window = line_bytes * (double)n2;
  const double budget = M.opt.sched_budget;  // default 2 MB of the 4 MiB per-XCD L2 (the rest: matrix stream, b/d/out lines); tests force tiling
  if (plane_window <= budget) return MG_OK;  // natural order already keeps the window in L2
  long long T = (long long)(budget / line_bytes);
  T = std::max<long long>(4, std::min<long long>(T, n2));
  std::vector<long long> key((size_t)nb);
  for (int b = 0; b < nb; ++b) {
    const long long r0 = h_blk[(size_t)b];
    const long long y = (r0 / n1) % n2, z = r0 / (n1 * n2);
    key[(size_t)b] = ((y / T) * n3 + z) * n2 + y;
  }
  std::vector<int> order((size_t)nb);
  for (int b = 0; b < nb; ++b) order[(size_t)b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });
  MG_TRY(sched.alloc((size_t)nb));
  HIP_TRY(hipMemcpy(sched.p, order.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice));
  has = true;
  return MG_OK;
}

// ---- small grid levels (mg_small.hpp) ----------------------------------------------------------------------------------------
// Everything is derived from the device's own CSR arrays (copied back once) and VERIFIED row by row; any row that does not fit
// leaves the operator on its other kernels.
static int small_download(const Csr& M, std::vector<int>& rp, std::vector<int>& ci, std::vector<double>& va) {
  rp.resize((size_t)M.n_rows + 1);
  ci.resize((size_t)std::max<long long>(M.nnz, 1));
  va.resize((size_t)std::max<long long>(M.nnz, 1));
  HIP_TRY(hipMemcpy(rp.data(), M.rowptr.p, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (M.nnz > 0) {
    HIP_TRY(hipMemcpy(ci.data(), M.colidx.p, (size_t)M.nnz * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(va.data(), M.val.p, (size_t)M.nnz * sizeof(double), hipMemcpyDeviceToHost));
  }
  return MG_OK;
}
static inline int small_code1(long long i, long long n) { return i == 0 ? 0 : (i == n - 1 ? 2 : 1); }
// A: square 27-point grid operator, relaxPrec constant over the rows of a position code
int build_small27(Csr& A, const long long grid[3], const double* d_dev, bool relax_set) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  A.sm_ok = false;
  A.sm_d_bound = nullptr;
  const long long n1 = grid[0], n2 = grid[1], n3 = grid[2], n = A.n_rows;
  if (A.opt.no_small || !A.set || n != A.n_cols || n1 < 2 || n2 < 2 || n3 < 1 || n1 * n2 * n3 != n || n > A.opt.small_max_rows || A.regular_cols >= 0) return MG_OK;
  if (A.nnz > 27 * n || n + 2 * n1 * n2 >= (1LL << 30)) return MG_OK;
  std::vector<int> rp, ci;
  std::vector<double> va, dh;
  MG_TRY(small_download(A, rp, ci, va));
  if (relax_set && d_dev) {
    dh.resize((size_t)n);
    HIP_TRY(hipMemcpy(dh.data(), d_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  }
  const long long P = n1 * n2;
  std::vector<double> rec(27 * 28, 0.0), cur(28);
  std::vector<char> seen(27, 0);
  for (long long row = 0; row < n; ++row) {
    const long long z = row / P, rem = row - z * P, y = rem / n1, x = rem - y * n1;
    const int code = (small_code1(z, n3) * 3 + small_code1(y, n2)) * 3 + small_code1(x, n1);
    std::fill(cur.begin(), cur.end(), 0.0);
    int last = -1;
    for (int k = rp[(size_t)row]; k < rp[(size_t)row + 1]; ++k) {
      const long long c = ci[(size_t)k], cz = c / P, cr = c - cz * P, cy = cr / n1, cx = cr - cy * n1;
      const long long dz = cz - z, dy = cy - y, dx = cx - x;
      if (dz < -1 || dz > 1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) return MG_OK;
      const int slot = (int)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
      if (slot <= last) return MG_OK;                              // (ascending columns: the order of the products)
      last = slot;
      cur[(size_t)slot] = va[(size_t)k];
    }
    cur[27] = dh.empty() ? 0.0 : dh[(size_t)row];
    double* q = rec.data() + (size_t)code * 28;
    if (!seen[(size_t)code]) {
      std::memcpy(q, cur.data(), 28 * sizeof(double));
      seen[(size_t)code] = 1;
    } else if (std::memcmp(q, cur.data(), 28 * sizeof(double)) != 0) {
      return MG_OK;                                                // rows of one position code differ: not a constant-coefficient grid operator
    }
  }
  MG_TRY(A.sm_rec.alloc(rec.size()));
  HIP_TRY(hipMemcpy(A.sm_rec.p, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
  A.sm = mgk::Small27Dev{A.sm_rec.p, (int)n1, (int)n2, (int)n3, (int)P, (int)n};
  A.sm_d_bound = dh.empty() ? nullptr : d_dev;
  A.sm_ok = true;
  if (A.opt.debug_format) std::fprintf(stderr, "[mg] small27: grid %lldx%lldx%lld (%lld rows)\n", n1, n2, n3, n);
  return MG_OK;
}
// R: rows = coarse grid gc, columns = fine grid gf; every entry a fine node (2i+dx, 2j+dy, 2k+dz), |d| <= 1.  An ordinary pair has
// gf = 2*gc - 1; an EMBEDDED pair (round 6: the sharded cycle's extended boxes) has gf = 2*m - 1 for a sub-box [o, o + m) of the coarse
// grid - the rows outside the sub-box are empty, (i, j, k) below are positions inside it.  The offset is read off the data: the first
// non-empty row is the sub-box's first node.
int build_small_restrict(Csr& R, const long long gf[3], const long long gc[3]) {
  if (R.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  R.smr_ok = false;
  R.waver_ok = false;
  const long long nc1 = gc[0], nc2 = gc[1], nc3 = gc[2], nf1 = gf[0], nf2 = gf[1], nf3 = gf[2];
  if (!R.set || nc1 < 2 || nc2 < 2 || nc3 < 1 || !(nf1 & 1) || !(nf2 & 1) || !(nf3 & 1)) return MG_OK;
  const long long m1 = (nf1 + 1) / 2, m2 = (nf2 + 1) / 2, m3 = (nf3 + 1) / 2;
  if (m1 < 2 || m2 < 2 || m1 > nc1 || m2 > nc2 || m3 > nc3) return MG_OK;
  if (nc1 * nc2 * nc3 != R.n_rows || nf1 * nf2 * nf3 != R.n_cols || R.regular_cols >= 0) return MG_OK;
  if (R.nnz > 27 * R.n_rows || R.n_cols + 2 * nf1 * nf2 >= (1LL << 30) || R.n_rows >= (1LL << 30)) return MG_OK;
  const bool embedded = m1 != nc1 || m2 != nc2 || m3 != nc3;
  // the lane-per-coarse-row kernel with its records serves the small levels (ordinary pairs); rows whose weights are
  // scale * 2^-(|dz|+|dy|+|dx|) throughout (R = scale * P' of the trilinear P) can take the wavefront form at any size (grid_wave_restrict)
  const bool want_small = !embedded && !R.opt.no_small && R.n_rows <= std::max(R.opt.small_max_rows, R.opt.small_r_max_rows);
  const bool want_wave = !R.opt.no_wave_restrict && R.n_rows >= R.opt.wave_restrict_min_rows;
  if (!want_small && !want_wave) return MG_OK;
  bool arith = true;
  double scale = 0.0;
  std::vector<int> rp, ci;
  std::vector<double> va;
  MG_TRY(small_download(R, rp, ci, va));
  const long long Pc = nc1 * nc2, Pf = nf1 * nf2;
  long long o1 = 0, o2 = 0, o3 = 0;
  if (embedded) {
    long long first = 0;
    while (first < R.n_rows && rp[(size_t)first + 1] == rp[(size_t)first]) ++first;
    if (first >= R.n_rows) return MG_OK;
    o3 = first / Pc; o2 = (first - o3 * Pc) / nc1; o1 = first - o3 * Pc - o2 * nc1;
    if (o1 + m1 > nc1 || o2 + m2 > nc2 || o3 + m3 > nc3) return MG_OK;
  }
  std::vector<double> rec(27 * 27, 0.0), cur(27);
  std::vector<char> seen(27, 0);
  for (long long row = 0; row < R.n_rows; ++row) {
    const long long kf = row / Pc, rem = row - kf * Pc, jf = rem / nc1, i_f = rem - jf * nc1;
    const long long k3 = kf - o3, j = jf - o2, i = i_f - o1;
    if (k3 < 0 || k3 >= m3 || j < 0 || j >= m2 || i < 0 || i >= m1) {       // outside the sub-box: an empty row
      if (rp[(size_t)row + 1] != rp[(size_t)row]) return MG_OK;
      continue;
    }
    const int code = (small_code1(k3, m3) * 3 + small_code1(j, m2)) * 3 + small_code1(i, m1);
    std::fill(cur.begin(), cur.end(), 0.0);
    int last = -1;
    for (int k = rp[(size_t)row]; k < rp[(size_t)row + 1]; ++k) {
      const long long c = ci[(size_t)k], cz = c / Pf, cr = c - cz * Pf, cy = cr / nf1, cx = cr - cy * nf1;
      const long long dz = cz - 2 * k3, dy = cy - 2 * j, dx = cx - 2 * i;
      if (dz < -1 || dz > 1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) return MG_OK;
      const int slot = (int)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
      if (slot <= last) return MG_OK;
      last = slot;
      cur[(size_t)slot] = va[(size_t)k];
    }
    if (arith) {       // every fine node of the 3 x 3 x 3 block that lies inside the grid, with the weight of its distance
      if (scale == 0.0) scale = cur[13];
      for (int s = 0; s < 27 && arith; ++s) {
        const long long dz = s / 9 - 1, dy = (s / 3) % 3 - 1, dx = s % 3 - 1;
        const bool in = 2 * k3 + dz >= 0 && 2 * k3 + dz < nf3 && 2 * j + dy >= 0 && 2 * j + dy < nf2 && 2 * i + dx >= 0 && 2 * i + dx < nf1;
        const double w = in ? scale * (dz ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0) : 0.0;
        arith = cur[(size_t)s] == w;
      }
    }
    double* q = rec.data() + (size_t)code * 27;
    if (!seen[(size_t)code]) {
      std::memcpy(q, cur.data(), 27 * sizeof(double));
      seen[(size_t)code] = 1;
    } else if (std::memcmp(q, cur.data(), 27 * sizeof(double)) != 0) {
      return MG_OK;
    }
  }
  if (embedded && !(arith && scale != 0.0)) return MG_OK;     // (an embedded pair has the wavefront form only)
  MG_TRY(R.smr_rec.alloc(rec.size()));
  HIP_TRY(hipMemcpy(R.smr_rec.p, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
  R.smr = mgk::SmallRDev{R.smr_rec.p, (int)nc1, (int)nc2, (int)nc3, (int)Pc, (int)R.n_rows, (int)nf1, (int)nf2, (int)nf3, (int)Pf, (int)R.n_cols,
                         (int)o1, (int)o2, (int)o3, (int)m1, (int)m2, (int)m3};
  R.smr_ok = want_small;
  R.waver_ok = want_wave && arith && scale != 0.0;
  R.waver_scale = scale;
  if (R.opt.debug_format) std::fprintf(stderr, "[mg] grid restriction: coarse grid %lldx%lldx%lld, sub-box %lldx%lldx%lld at (%lld,%lld,%lld)%s%s\n", nc1, nc2, nc3, m1, m2, m3,
                                       o1, o2, o3, R.smr_ok ? ", records" : "", R.waver_ok ? ", wavefront form" : "");
  return MG_OK;
}
// P: rows = fine grid gf, columns = coarse grid gc; the stored operator must BE the full-weighting interpolation (weight 1 from the
// coincident coarse node, 1/2 from both neighbours of an odd coordinate; GeometricTransferOperators.jl:27-29) from the coarse grid
// (gf = 2*gc - 1) or from a sub-box [o, o + m) of it (gf = 2*m - 1, embedded pair: the offset is the column of the first row's one entry)
int build_small_prolong(Csr& Pm, const long long gf[3], const long long gc[3]) {
  if (Pm.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  Pm.smp_ok = false;
  Pm.cellp_ok = false;
  const long long nc1 = gc[0], nc2 = gc[1], nc3 = gc[2], nf1 = gf[0], nf2 = gf[1], nf3 = gf[2];
  if (!Pm.set || nc1 < 2 || nc2 < 2 || nc3 < 1 || !(nf1 & 1) || !(nf2 & 1) || !(nf3 & 1)) return MG_OK;
  const long long m1 = (nf1 + 1) / 2, m2 = (nf2 + 1) / 2, m3 = (nf3 + 1) / 2;
  if (m1 < 2 || m2 < 2 || m1 > nc1 || m2 > nc2 || m3 > nc3) return MG_OK;
  if (nf1 * nf2 * nf3 != Pm.n_rows || nc1 * nc2 * nc3 != Pm.n_cols || Pm.regular_cols >= 0) return MG_OK;
  if (Pm.n_rows >= (1LL << 30) || Pm.n_cols >= (1LL << 30)) return MG_OK;
  const bool embedded = m1 != nc1 || m2 != nc2 || m3 != nc3;
  // the lane-per-fine-row kernel serves the small levels, the lane-per-coarse-cell kernel every size (the check below is the same)
  const bool want_small = !Pm.opt.no_small && Pm.n_rows <= std::max(Pm.opt.small_max_rows, Pm.opt.small_p_max_rows);
  const bool want_cell = !Pm.opt.no_cell_prolong;
  if (!want_small && !want_cell) return MG_OK;
  std::vector<int> rp, ci;
  std::vector<double> va;
  MG_TRY(small_download(Pm, rp, ci, va));
  const long long Pc = nc1 * nc2, Pf = nf1 * nf2;
  long long o1 = 0, o2 = 0, o3 = 0;
  if (embedded) {
    if (rp[1] - rp[0] != 1) return MG_OK;
    const long long first = ci[(size_t)rp[0]];
    o3 = first / Pc; o2 = (first - o3 * Pc) / nc1; o1 = first - o3 * Pc - o2 * nc1;
    if (o1 + m1 > nc1 || o2 + m2 > nc2 || o3 + m3 > nc3) return MG_OK;
  }
  for (long long row = 0; row < Pm.n_rows; ++row) {
    const long long z = row / Pf, rem = row - z * Pf, y = rem / nf1, x = rem - y * nf1;
    const int oz = (int)(z & 1), oy = (int)(y & 1), ox = (int)(x & 1);
    const double w = (oz ? 0.5 : 1.0) * (oy ? 0.5 : 1.0) * (ox ? 0.5 : 1.0);
    const long long c0 = ((z >> 1) + o3) * Pc + ((y >> 1) + o2) * nc1 + (x >> 1) + o1;
    int k = rp[(size_t)row];
    for (int s = 0; s < 8; ++s) {
      const int dz = (s >> 2) & 1, dy = (s >> 1) & 1, dx = s & 1;
      if (dz > oz || dy > oy || dx > ox) continue;
      if (k >= rp[(size_t)row + 1] || ci[(size_t)k] != c0 + dz * Pc + dy * nc1 + dx || va[(size_t)k] != w) return MG_OK;
      ++k;
    }
    if (k != rp[(size_t)row + 1]) return MG_OK;
  }
  Pm.smp = mgk::SmallPDev{(int)nf1, (int)nf2, (int)nf3, (int)Pf, (int)Pm.n_rows, (int)nc1, (int)nc2, (int)nc3, (int)Pc, (int)Pm.n_cols,
                          (int)o1, (int)o2, (int)o3, (int)m1, (int)m2, (int)m3};
  Pm.smp_ok = want_small;
  Pm.cellp_ok = want_cell;
  if (Pm.opt.debug_format) std::fprintf(stderr, "[mg] grid prolongation: fine grid %lldx%lldx%lld from the sub-box at (%lld,%lld,%lld) of %lldx%lldx%lld\n", nf1, nf2, nf3, o1, o2, o3, nc1, nc2, nc3);
  return MG_OK;
}

// Band-27 form of a variable-coefficient 27-point grid operator (no row classes, no 7-point band form, not served by the small-level
// records): the planar arrays are (re)filled on the device from the CSR values; a row that does not fit drops the form.
int build_band27(Csr& A, const long long grid[3]) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  const long long n1 = grid[0], n2 = grid[1], n3 = grid[2], n = A.n_rows;
  const bool want = !A.opt.no_band27 && A.set && !A.has_rc && !A.rm3_var && !A.sm_ok && n == A.n_cols && n1 >= 2 && n2 >= 2 && n3 >= 1 && n1 * n2 * n3 == n &&
                    n <= A.opt.band27_max_rows && A.regular_cols < 0 && A.max_row_nnz <= 27 && A.max_row_nnz > 7 && n + 2 * n1 * n2 < (1LL << 30);
  if (!want) {
    A.b27_ok = false;
    A.b27_val.release();
    return MG_OK;
  }
  const long long stride = ((n + 15) & ~15LL) + ((n1 * n2 + n1 + 1 + 15) & ~15LL);   // (zeros behind every slot: the symmetric reads of the first rows)
  if (A.b27_val.n != (size_t)(27 * stride)) {
    MG_TRY(A.b27_val.alloc((size_t)(27 * stride)));
    HIP_TRY(hipMemset(A.b27_val.p, 0, A.b27_val.bytes()));
  }
  if (A.b27_flag.n != 1) MG_TRY(A.b27_flag.alloc(1));
  HIP_TRY(hipMemset(A.b27_flag.p, 0, sizeof(int)));
  hipLaunchKernelGGL(mgk::band27_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, A.dev(), (int)n1, (int)n2, (int)n3, A.b27_val.p, stride, A.b27_flag.p);
  HIP_TRY(hipGetLastError());
  int bad = 0;
  HIP_TRY(hipMemcpy(&bad, A.b27_flag.p, sizeof(int), hipMemcpyDeviceToHost));
  if (bad) {
    A.b27_ok = false;
    A.b27_val.release();
    return MG_OK;
  }
  A.b27 = mgk::Band27Dev{A.b27_val.p, stride, (int)n1, (int)n2, (int)n3, (int)(n1 * n2), (int)n, 0};
  if (!A.opt.no_band_sym) {      // symmetric values (Galerkin coarse operators of a symmetric fine one)?
    HIP_TRY(hipMemset(A.b27_flag.p, 0, sizeof(int)));
    hipLaunchKernelGGL(mgk::band27_sym_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, A.b27, A.opt.band_sym_tol ? 8.8817841970012523e-16 : 0.0, A.b27_flag.p);
    HIP_TRY(hipGetLastError());
    int asym = 1;
    HIP_TRY(hipMemcpy(&asym, A.b27_flag.p, sizeof(int), hipMemcpyDeviceToHost));
    A.b27.sym = asym == 0 ? 1 : 0;
  }
  A.b27_ok = true;
  if (A.opt.debug_format) std::fprintf(stderr, "[mg] band-27: grid %lldx%lldx%lld (%lld rows, %.1f MB of planar values%s)\n", n1, n2, n3, n, 216.0e-6 * (double)stride, A.b27.sym ? ", symmetric reads" : "");
  return MG_OK;
}

int alloc_scratch(mg_hierarchy* h) {
  const long long k = h->nrhs;
  if (h->coarse_lu) MG_TRY(h->luWork.alloc((size_t)h->n_coarse * (size_t)k));
  if (h->coarse_lu && std::max(h->luML, h->luMU) > 0) MG_TRY(h->luTail.alloc((size_t)std::max(h->luML, h->luMU) * (size_t)k));
  if (!h->opt.no_sched) {
    for (int l = 0; l < (int)h->nlevels; ++l) {
      Level& L = h->lev[(size_t)l];
      MG_TRY(build_schedule(L.A, L.grid, k));
      MG_TRY(build_staged(L.A, L.grid));
      MG_TRY(build_schedule(L.P, L.grid, k));
      if (l + 1 < (int)h->nlevels) MG_TRY(build_schedule(L.R, h->lev[(size_t)l + 1].grid, k));
      // (the single-vector forms of P and R also serve a block that is solved column by column: solve_dev_columns)
      if (l + 1 < (int)h->nlevels) MG_TRY(build_winp(L.P, L.grid, h->lev[(size_t)l + 1].grid));
      if (l + 1 < (int)h->nlevels) MG_TRY(build_marchr(L.R, L.grid, h->lev[(size_t)l + 1].grid));
    }
  }
  for (int l = 0; l < (int)h->nlevels; ++l) {   // small grid levels: the one-trip kernels (mg_small.hpp)
    Level& L = h->lev[(size_t)l];
    const bool last = l + 1 >= (int)h->nlevels;
    MG_TRY(build_small27(L.A, L.grid, L.d.p, L.relax_set && !last));
    MG_TRY(build_band27(L.A, L.grid));
    if (!last) {
      MG_TRY(build_small_restrict(L.R, L.grid, h->lev[(size_t)l + 1].grid));
      MG_TRY(build_small_prolong(L.P, L.grid, h->lev[(size_t)l + 1].grid));
    }
  }
  h->lane0.release_vectors();   // (every finalize starts from zeroed vectors)
  MG_TRY(h->lane0.alloc(h, k, /*fine=*/true));
  long long nmax = 0;
  for (int l = 0; l < (int)h->nlevels; ++l) {
    Level& L = h->lev[l];
    const size_t len = (size_t)L.n * (size_t)k;
    nmax = std::max(nmax, L.n);
    // FGMRESmem (MGsetup.jl:190-215): memRelax[l] for Jac-GMRES, memKcycle for levels 2..nl-1 of a K-cycle
    L.relaxZ.release();
    L.relaxAZ.release();
    L.kZ.release();
    L.kAZ.release();
    if (h->relax_type == 1 && l < (int)h->nlevels - 1) {
      L.relax_inner = std::max<long long>(1, std::max(L.npre, L.npost));
      MG_TRY(L.relaxZ.alloc(len * (size_t)L.relax_inner));
      MG_TRY(L.relaxAZ.alloc(len * (size_t)L.relax_inner));
    }
    if (h->cycle == 'K' && l > 0 && l < (int)h->nlevels - 1) {
      MG_TRY(L.kZ.alloc(len * 2));
      MG_TRY(L.kAZ.alloc(len * 2));
    }
  }
  // store sink of the tile-form passes, at its largest size (12 stores x 32 slabs x 1024 lanes = 3 MB): never (re)allocated
  // on the launch path - a launch may sit inside a stream capture, and earlier graphs hold the pointer
  if (h->m3sink.n < M3_SINK_DOUBLES) MG_TRY(h->m3sink.alloc(M3_SINK_DOUBLES));
  // host-pointer API staging (fine level) + transpose scratch (any level, for mg_spmv)
  MG_TRY(h->stage_b.alloc((size_t)nmax * k));
  MG_TRY(h->stage_x.alloc((size_t)nmax * k));
  MG_TRY(h->stage_t.alloc((size_t)nmax * k));
  HIP_TRY(hipMemset(h->stage_b.p, 0, h->stage_b.bytes()));
  HIP_TRY(hipMemset(h->stage_x.p, 0, h->stage_x.bytes()));
  HIP_TRY(hipMemset(h->stage_t.p, 0, h->stage_t.bytes()));
  h->last_b = nullptr;
  h->last_x = nullptr;
  return MG_OK;
}

// Dictionary-code the column indices: per row (first column, pattern id), pattern = cols - cols[0].
// Adopted only if it is a clear win: <= 65535 patterns and a dictionary below 1/16 of the index array.
int build_patterns(Csr* M, const std::vector<int>& rp, const std::vector<int>& ci) {
  M->has_pat = false;
  const long long n = M->n_rows;
  // short rows (full-weighting P: 1..8 entries) gain little index traffic and pay the extra dependent
  // descriptor loads: measured +18 % time on C2's prolongation -> keep plain CSR below 5 entries per row
  if (M->nnz < 5 * n) return MG_OK;
  std::vector<int> first((size_t)n, 0);
  std::vector<unsigned short> pid((size_t)n, 0);
  std::vector<int> pptr(1, 0), poff;
  std::unordered_map<unsigned long long, std::vector<int>> table;  // hash -> pattern ids
  const size_t dict_cap = (size_t)std::max<long long>(4096, M->nnz / 16);
  for (long long i = 0; i < n; ++i) {
    const int s = rp[(size_t)i], e = rp[(size_t)i + 1];
    const int f = (e > s) ? ci[(size_t)s] : 0;
    first[(size_t)i] = f;
    unsigned long long hsh = 1469598103934665603ull ^ (unsigned long long)(e - s);
    for (int k = s; k < e; ++k) {
      hsh ^= (unsigned long long)(unsigned int)(ci[(size_t)k] - f);
      hsh *= 1099511628211ull;
    }
    std::vector<int>& cand = table[hsh];
    int found = -1;
    for (int id : cand) {
      const int ps = pptr[(size_t)id], len = pptr[(size_t)id + 1] - ps;
      if (len != e - s) continue;
      bool same = true;
      for (int k = 0; k < len; ++k)
        if (poff[(size_t)ps + k] != ci[(size_t)s + k] - f) { same = false; break; }
      if (same) { found = id; break; }
    }
    if (found < 0) {
      found = (int)pptr.size() - 1;
      if (found >= 65535 || poff.size() + (size_t)(e - s) > dict_cap) return MG_OK;  // not a grid-like operator
      for (int k = s; k < e; ++k) poff.push_back(ci[(size_t)k] - f);
      pptr.push_back((int)poff.size());
      cand.push_back(found);
    }
    pid[(size_t)i] = (unsigned short)found;
  }
  if (poff.empty()) poff.push_back(0);
  MG_TRY(M->firstcol.alloc(first.size()));
  MG_TRY(M->pat.alloc(pid.size()));
  MG_TRY(M->pat_ptr.alloc(pptr.size()));
  MG_TRY(M->pat_off.alloc(poff.size()));
  HIP_TRY(hipMemcpy(M->firstcol.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->pat.p, pid.data(), pid.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->pat_ptr.p, pptr.data(), pptr.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->pat_off.p, poff.data(), poff.size() * sizeof(int), hipMemcpyHostToDevice));
  M->npat = (long long)pptr.size() - 1;
  M->dict_entries = (long long)poff.size();
  M->has_pat = true;
  // run-length form of the row descriptors, per row block
  {
    if (M->opt.no_runs) return MG_OK;
    // the descriptors are 10 B/row: worth compressing next to 56 B/row of values (7-point), not next to
    // 216 B/row (27-point), where the run lookup costs more than it saves (measured -5 % / +4 %)
    if (M->nnz >= 16 * n) return MG_OK;
  }
  const int nb = M->nblocks;
  std::vector<int> rptr((size_t)nb + 1, 0), runs;
  for (int b = 0; b < nb; ++b) {
    const int r0 = M->h_blk_row[(size_t)b], r1 = M->h_blk_row[(size_t)b + 1];
    const size_t mark = runs.size();
    int count = 0;
    bool ok = true;
    int i = r0;
    while (i < r1) {
      const int pidv = pid[(size_t)i], f0 = first[(size_t)i];
      int stride = 0, j = i + 1;
      if (j < r1 && pid[(size_t)j] == pidv) {
        stride = first[(size_t)j] - f0;
        while (j < r1 && pid[(size_t)j] == pidv && first[(size_t)j] == f0 + (j - i) * stride) ++j;
      }
      if (++count > mgk::MAXRUNS) { ok = false; break; }
      runs.push_back(i - r0);
      runs.push_back(pidv);
      runs.push_back(f0);
      runs.push_back(stride);
      runs.push_back(rp[(size_t)i]);
      i = j;
    }
    const bool longrow = (r1 - r0 == 1) && (rp[(size_t)r1] - rp[(size_t)r0] > mgk::CHUNK - 2);
    if (!ok || longrow) runs.resize(mark);  // this block keeps the per-row descriptors
    rptr[(size_t)b + 1] = (int)(runs.size() / 5);
  }
  if (runs.empty()) return MG_OK;
  MG_TRY(M->run_ptr.alloc(rptr.size()));
  MG_TRY(M->runs.alloc(runs.size()));
  HIP_TRY(hipMemcpy(M->run_ptr.p, rptr.data(), rptr.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->runs.p, runs.data(), runs.size() * sizeof(int), hipMemcpyHostToDevice));
  M->nruns_total = (long long)(runs.size() / 5);
  M->has_runs = true;
  return MG_OK;
}

// Row classes: rows with identical column offsets (relative to the row's first column) AND bit-identical values.
// Accepted when the operator really is that redundant: at most 65535 classes and a dictionary of at most
// min(nnz/16, 2^18) entries (3 MiB: L2-resident).  Anything else keeps the streaming formats.  Lossless.
int build_rowclasses_try(Csr* M, const int* rp, const int* ci, const double* val, bool implicit) {
  M->drop_rc();
  const long long n = M->n_rows;
  if (n < 1 || M->nnz < 1) return MG_OK;
  bool pair_choice = false;
  const size_t cap = (size_t)std::min<long long>(1LL << 18, std::max<long long>(64, M->nnz / 16));
  // Phase 1: classify every row (raw classes, unbounded ids).  Mostly regular operators - a grid operator whose
  // rows were renumbered near sub-domain faces, irregular boundaries - have a few popular classes and a tail of
  // singletons; give up only when the operator is irregular throughout.
  const size_t raw_cls_cap = (size_t)std::max<long long>(65535, n / 8);
  const size_t raw_ent_cap = (size_t)std::max<long long>((long long)cap, M->nnz / 4);
  std::vector<int> first((size_t)n, 0), rptr(1, 0), roff, rdelta, rid((size_t)n, 0);
  std::vector<double> rval;
  std::unordered_map<unsigned long long, std::vector<int>> table;
  for (long long i = 0; i < n; ++i) {
    const int s = rp[(size_t)i], e = rp[(size_t)i + 1];
    const int f = (e > s) ? ci[(size_t)s] : 0;
    first[(size_t)i] = f;
    if (M->regular_cols >= 0 && (i >= M->reg_rows() || (e > s && ci[(size_t)e - 1] >= M->regular_cols))) {
      rid[(size_t)i] = -1;   // halo row, or a row that reads the halo (columns are sorted): forced exception row
      continue;
    }
    unsigned long long hsh = 1469598103934665603ull ^ (unsigned long long)(e - s);
    const int dlt = (int)(f - i);
    if (implicit) {
      hsh ^= (unsigned long long)(unsigned int)dlt;
      hsh *= 1099511628211ull;
    }
    for (int k = s; k < e; ++k) {
      unsigned long long bits;
      std::memcpy(&bits, &val[(size_t)k], 8);
      hsh ^= (unsigned long long)(unsigned int)(ci[(size_t)k] - f);
      hsh *= 1099511628211ull;
      hsh ^= bits;
      hsh *= 1099511628211ull;
    }
    std::vector<int>& cand = table[hsh];
    int found = -1;
    for (int id : cand) {
      const int ps = rptr[(size_t)id], len = rptr[(size_t)id + 1] - ps;
      if (len != e - s) continue;
      if (implicit && rdelta[(size_t)id] != dlt) continue;
      bool same = true;
      for (int k = 0; k < len && same; ++k)
        same = roff[(size_t)ps + k] == ci[(size_t)s + k] - f &&
               std::memcmp(&rval[(size_t)ps + k], &val[(size_t)s + k], 8) == 0;
      if (same) { found = id; break; }
    }
    if (found < 0) {
      found = (int)rptr.size() - 1;
      if ((size_t)found >= raw_cls_cap || roff.size() + (size_t)(e - s) > raw_ent_cap) return MG_OK;  // irregular
      for (int k = s; k < e; ++k) {
        roff.push_back(ci[(size_t)k] - f);
        rval.push_back(val[(size_t)k]);
      }
      rptr.push_back((int)roff.size());
      rdelta.push_back(dlt);
      cand.push_back(found);
    }
    rid[(size_t)i] = found;
    // early exit for operators that are irregular from the start (SA-AMG levels: 2.5 G non-zeros in C3's hierarchy
    // would otherwise be hashed up to the caps above): more than half of the first 8192 rows distinct
    if (i == 8191 && rptr.size() - 1 > 4096) return MG_OK;
  }
  table.clear();
  // Phase 2: keep the most frequent classes that fit the id width and the dictionary cap; rows of any other class
  // are EXCEPTION rows (class id 0xFFFF): the row-class kernels skip them and csr_rows_spmv computes them from the
  // CSR arrays.  Accepted when the kept classes cover enough rows (MG_ROWCLASS_MIN_COVER, default 0.9).
  const size_t nraw = rptr.size() - 1;
  std::vector<long long> freq(nraw, 0);
  for (long long i = 0; i < n; ++i)
    if (rid[(size_t)i] >= 0) freq[(size_t)rid[(size_t)i]]++;
  std::vector<int> order(nraw);
  for (size_t c = 0; c < nraw; ++c) order[c] = (int)c;
  std::sort(order.begin(), order.end(), [&](int x, int y) { return freq[(size_t)x] != freq[(size_t)y] ? freq[(size_t)x] > freq[(size_t)y] : x < y; });
  std::vector<int> remap(nraw, 0xFFFF), cptr(1, 0), coff, cdelta;
  std::vector<double> cval;
  long long covered = 0, nsingle = 0;
  const long long keep_single = M->opt.rowclass_keep_singletons;   // default 1024; tests
  for (size_t c = 0; c < nraw; ++c) nsingle += freq[c] == 1;
  for (size_t t = 0; t < nraw && cptr.size() - 1 < 65535; ++t) {
    const int c = order[t];
    const int ps = rptr[(size_t)c], len = rptr[(size_t)c + 1] - ps;
    // a few singletons (the corners of a box) may as well live in the dictionary; a long tail of them (rows next
    // to sub-domain faces) becomes exception rows
    if (freq[(size_t)c] < 2 && nsingle > keep_single) break;
    if (coff.size() + (size_t)len > cap) break;
    remap[(size_t)c] = (int)cptr.size() - 1;
    coff.insert(coff.end(), roff.begin() + ps, roff.begin() + ps + len);
    cval.insert(cval.end(), rval.begin() + ps, rval.begin() + ps + len);
    cptr.push_back((int)coff.size());
    cdelta.push_back(rdelta[(size_t)c]);
    covered += freq[(size_t)c];
  }
  {
    const double min_cover = M->opt.rowclass_min_cover;
    const double nreg = (double)M->reg_rows();
    if (cptr.size() < 2 || (double)covered < min_cover * nreg) return MG_OK;
  }
  std::vector<unsigned short> cid((size_t)n, 0);
  std::vector<int> exc;
  for (long long i = 0; i < n; ++i) {
    const int c = rid[(size_t)i] >= 0 ? remap[(size_t)rid[(size_t)i]] : 0xFFFF;
    cid[(size_t)i] = (unsigned short)c;
    // (the empty halo rows of a padded local operator are never computed: not even exception rows)
    if (c == 0xFFFF && i < M->reg_rows()) exc.push_back((int)i);
  }
  { std::vector<int>().swap(rid); std::vector<int>().swap(roff); std::vector<double>().swap(rval); }
  if (coff.empty()) { coff.push_back(0); cval.push_back(0.0); }
  {
    // The kernel serves one class per waterfall pass: it only pays when a wavefront's 64 consecutive rows hold few
    // classes.  Measured on C2: levels of 35 937 rows and fewer (every wave sees a dozen classes, and the whole level
    // is L2-resident anyway) ran 3x slower than with the streaming kernels -> require <= 4 classes per wave on
    // average, and enough rows for the matrix stream to matter.
    const long long min_rows = M->opt.rowclass_min_rows, max_passes = M->opt.rowclass_max_passes;   // 100000 / 4; tests, A/B
    if (n < min_rows) return MG_OK;
    long long passes = 0, waves = 0;
    for (long long w0 = 0; w0 < n; w0 += 64) {
      unsigned short seen[64];
      int ns = 0;
      const long long w1 = std::min(n, w0 + 64);
      for (long long i = w0; i < w1; ++i) {
        if (cid[(size_t)i] == 0xFFFF) continue;   // exception rows cost no pass
        bool dup = false;
        for (int t = 0; t < ns; ++t)
          if (seen[t] == cid[(size_t)i]) { dup = true; break; }
        if (!dup) seen[ns++] = cid[(size_t)i];
      }
      passes += ns;
      ++waves;
    }
    if (passes > max_passes * waves) return MG_OK;
    // two consecutive rows per lane when that roughly halves the passes (classes alternating row by row)
    long long passes2 = 0;
    for (long long w0 = 0; w0 < n; w0 += 128) {
      unsigned short seen[128];
      int ns = 0;
      const long long w1 = std::min(n, w0 + 128);
      for (long long i = w0; i < w1; ++i) {
        if (cid[(size_t)i] == 0xFFFF) continue;
        bool dup = false;
        for (int t = 0; t < ns; ++t)
          if (seen[t] == cid[(size_t)i]) { dup = true; break; }
        if (!dup) seen[ns++] = cid[(size_t)i];
      }
      passes2 += ns;
    }
    // (only where a wave really holds alternating classes: uniform operators measured slower this way, R1 70 -> 84 us)
    // and only on large operators - C2's level 3 (65^3 rows, 4 classes per wave) ran 30 % slower paired
    const long long pair_min = M->opt.pair_min_rows;
    pair_choice = !M->opt.no_pair && n >= pair_min && 2 * passes >= 3 * waves && 10 * passes2 <= 7 * passes;
  }
  if (cdelta.empty()) cdelta.push_back(0);
  if (!implicit) MG_TRY(M->rc_first.alloc(first.size()));
  MG_TRY(M->rc_delta.alloc(cdelta.size()));
  HIP_TRY(hipMemcpy(M->rc_delta.p, cdelta.data(), cdelta.size() * sizeof(int), hipMemcpyHostToDevice));
  MG_TRY(M->rc_cls.alloc(cid.size()));
  MG_TRY(M->rc_ptr.alloc(cptr.size()));
  MG_TRY(M->rc_off.alloc(coff.size()));
  MG_TRY(M->rc_val.alloc(cval.size()));
  if (!implicit) HIP_TRY(hipMemcpy(M->rc_first.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->rc_cls.p, cid.data(), cid.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->rc_ptr.p, cptr.data(), cptr.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->rc_off.p, coff.data(), coff.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->rc_val.p, cval.data(), cval.size() * sizeof(double), hipMemcpyHostToDevice));
  M->rc_ncls = (long long)cptr.size() - 1;
  M->rc_entries = (long long)coff.size();
  M->rc_nexc = (int)exc.size();
  if (!exc.empty()) {
    MG_TRY(M->rc_exc.alloc(exc.size()));
    HIP_TRY(hipMemcpy(M->rc_exc.p, exc.data(), exc.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  M->has_rc = true;
  M->rc_implicit = implicit;
  M->rc_pair = pair_choice;
  M->h_rc_ptr = cptr;
  M->h_rc_off = coff;
  M->h_rc_delta = cdelta;
  M->rc_maxlen = 0;
  for (size_t c = 0; c + 1 < cptr.size(); ++c) M->rc_maxlen = std::max(M->rc_maxlen, cptr[c + 1] - cptr[c]);
  if (implicit) {   // LDS-window kernel: do the windows of the most frequent class fit for a full workgroup of rows?
    std::vector<long long> cnt(cptr.size() - 1, 0);
    for (long long i = 0; i < n; ++i)
      if (cid[(size_t)i] != 0xFFFF) cnt[cid[(size_t)i]]++;
    const size_t cm = (size_t)(std::max_element(cnt.begin(), cnt.end()) - cnt.begin());
    M->rc_major = (int)cm;
    const int ps = cptr[cm], len = cptr[cm + 1] - ps;
    // MG_STAGE_MIN_LEN: shortest class worth staging (A/B switch; measured on C2, profiles/r01_nt_ab.md:
    // -25 % on the 27-point levels, -5 % on the 7-point one with the spill-free tile kernel)
    const long long min_len = M->opt.stage_min_len;
    // small levels are latency-bound and faster on the plain kernel (C2 level 3, 65^3 rows: 15 us against 23 us)
    const long long min_wg = M->opt.window_min_wg;
    bool ok = !M->opt.no_window && len >= min_len && len <= mgk::RW_MAXLEN && 2 * cnt[cm] >= n &&
              (n + mgk::RW_ROWS - 1) / mgk::RW_ROWS >= min_wg;
    if (ok) {
      const long long W = mgk::RW_ROWS;
      std::vector<int> meta(mgk::RW_META_HDR, 0), ivs;
      std::unordered_map<long long, int> lb_of_shift;   // staged shift (delta + off) -> LDS index
      const long long dcm = cdelta[cm];
      long long base = 0, o_start = coff[(size_t)ps], o_end = o_start;
      for (int k = 0; k < len; ++k) {
        const long long off = coff[(size_t)ps + k];
        if (k > 0 && off > o_end + W) {   // a new window (offsets ascend: CSR rows are sorted)
          ivs.push_back((int)o_start);
          ivs.push_back((int)(o_end - o_start + W));
          ivs.push_back((int)base);
          base += o_end - o_start + W;
          o_start = off;
        }
        o_end = off;
        lb_of_shift[dcm + off] = (int)(base + (off - o_start));
      }
      ivs.push_back((int)o_start);
      ivs.push_back((int)(o_end - o_start + W));
      ivs.push_back((int)base);
      base += o_end - o_start + W;
      const int nint = (int)(ivs.size() / 3);
      ok = base <= mgk::RW_CAP && nint <= mgk::RW_MAXINT;
      if (ok) {
        meta[0] = (int)cm;
        meta[1] = nint;
        auto it0 = lb_of_shift.find(0);
        meta[2] = it0 == lb_of_shift.end() ? -1 : it0->second;
        meta[3] = (int)base;
        meta.insert(meta.end(), ivs.begin(), ivs.end());
        // every dictionary entry of every class: the LDS index of its shift, or -1 (gathers from global memory)
        std::vector<int> lbs(coff.size(), -1);
        for (size_t c = 0; c + 1 < cptr.size(); ++c)
          for (int k = cptr[c]; k < cptr[c + 1]; ++k) {
            auto it = lb_of_shift.find((long long)cdelta[c] + coff[(size_t)k]);
            if (it != lb_of_shift.end()) lbs[(size_t)k] = it->second;
          }
        MG_TRY(M->rw_meta.alloc(meta.size()));
        HIP_TRY(hipMemcpy(M->rw_meta.p, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice));
        MG_TRY(M->rw_lb.alloc(lbs.size()));
        HIP_TRY(hipMemcpy(M->rw_lb.p, lbs.data(), lbs.size() * sizeof(int), hipMemcpyHostToDevice));
        M->rw_doubles = (int)base;
      }
    }
    M->rc_window = ok;
  }
  M->h_cls.swap(cid);
  return MG_OK;
}
// Square operators first try the form without a first-column stream (the class also fixes first column - row).
int build_rowclasses(Csr* M, const int* rp, const int* ci, const double* val) {
  if (M->n_rows == M->n_cols) {
    if (!M->opt.no_implicit_first) {
      MG_TRY(build_rowclasses_try(M, rp, ci, val, true));
      if (M->has_rc) return MG_OK;
    }
  }
  return build_rowclasses_try(M, rp, ci, val, false);
}
// relaxPrec constant per class (d = omega/a_ii and a_ii is part of the class): keep it in the dictionary
// relaxPrec constant over every dictionary class (omega / a_ii is, by construction): the fused sweep can read it from the
// dictionary instead of streaming 8 B/row.  d_dev: device vector over the operator's regular rows.
int derive_class_d_csr(Csr& A, const double* d_dev, size_t n_d) {
  if (A.wide) return MG_OK;   // (64-bit row pointers: the streaming kernels only)
  A.rc_has_d = false;
  A.d_bound = nullptr;
  const size_t nreg = (size_t)(A.regular_cols >= 0 ? A.regular_cols : A.n_rows);
  if (!A.has_rc || A.h_cls.size() != (size_t)A.n_rows || n_d != nreg || !d_dev) return MG_OK;
  if (A.opt.no_class_d) return MG_OK;
  std::vector<double> hd(nreg), dc((size_t)A.rc_ncls, 0.0);
  std::vector<char> seen((size_t)A.rc_ncls, 0);
  HIP_TRY(hipMemcpy(hd.data(), d_dev, hd.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < hd.size(); ++i) {
    const unsigned short c = A.h_cls[i];
    if (c == 0xFFFF) continue;   // exception rows read d from memory (csr_rows_spmv, xpdr_cls_kernel)
    if (!seen[c]) { seen[c] = 1; dc[c] = hd[i]; }
    else if (std::memcmp(&dc[c], &hd[i], 8) != 0) return MG_OK;   // not class-constant: keep streaming d
  }
  MG_TRY(A.rc_d.alloc(dc.size()));
  HIP_TRY(hipMemcpy(A.rc_d.p, dc.data(), dc.size() * sizeof(double), hipMemcpyHostToDevice));
  A.rc_has_d = true;
  A.d_bound = d_dev;
  return MG_OK;
}
int derive_class_d(Level& L) { return derive_class_d_csr(L.A, L.d.p, L.d.n); }
// New values on the stored pattern (mg_replace_values_FP64, mg_rap_FP64): the classes are re-derived from the host
// pattern kept for that purpose; an operator that is no longer redundant falls back to the streaming kernels.
int refresh_rowclasses(Csr* M, const double* val) {
  if (M->wide) return MG_OK;
  if (!M->has_rc) return MG_OK;
  if (M->h_rp.size() != (size_t)M->n_rows + 1) { M->drop_rc(); return MG_OK; }
  return build_rowclasses(M, M->h_rp.data(), M->h_ci.data(), val);
}

// Operators of >= 2^31 - 4096 non-zeros (the reference is Int64 throughout, Multigrid.jl:19; SURVEY section 7: "int64-capable or guarded"):
// 64-bit row pointers, 32-bit column indices (dimensions stay < 2^31), row blocks for csr_stream_spmv - nothing else is built: such an
// operator is streamed (one right-hand side), by csr_longrow_spmv where its rows average >= longrow_min_avg entries.
int upload_csr_wide(Csr* M, const Options& opt, long long n_rows, long long n_cols, const long long* colptr, const long long* rowval,
                    const double* nzval, long long nnz) {
  std::vector<long long> rp((size_t)n_rows + 1);
  for (long long i = 0; i <= n_rows; ++i) {
    const long long v = colptr[i] - 1;
    if (v < 0 || v > nnz || (i > 0 && v < rp[(size_t)i - 1])) return fail(MG_ERR_INVALID, "colptr is not a monotone 1-based pointer array at %lld", i);
    rp[(size_t)i] = v;
  }
  const size_t pad = 2 * mgk::BLK;
  M->release();
  M->opt = opt;
  M->regular_cols = -1;
  M->regular_rows = -1;
  M->n_rows = n_rows;
  M->n_cols = n_cols;
  M->nnz = nnz;
  M->wide = true;
  MG_TRY(M->colidx.alloc((size_t)nnz + pad));
  MG_TRY(M->val.alloc((size_t)nnz + pad));
  {   // column indices in slices (a 2^31-entry host copy would be 8.6 GB)
    const long long SL = 1LL << 26;
    std::vector<int> ci((size_t)std::min<long long>(SL, std::max<long long>(nnz, 1)));
    for (long long k0 = 0; k0 < nnz; k0 += SL) {
      const long long m = std::min(SL, nnz - k0);
      for (long long k = 0; k < m; ++k) {
        const long long c = rowval[k0 + k] - 1;
        if (c < 0 || c >= n_cols) return fail(MG_ERR_INVALID, "rowval[%lld]=%lld outside 1..%lld", k0 + k + 1, rowval[k0 + k], n_cols);
        ci[(size_t)k] = (int)c;
      }
      HIP_TRY(hipMemcpy(M->colidx.p + k0, ci.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemset(M->colidx.p + nnz, 0, pad * sizeof(int)));
  }
  HIP_TRY(hipMemset(M->val.p + nnz, 0, pad * sizeof(double)));
  HIP_TRY(hipMemcpy(M->val.p, nzval, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  // row blocks as upload_csr cuts them: consecutive rows, <= MAXROWS rows and an (even-aligned) nnz span <= CHUNK
  std::vector<int> blk;
  blk.push_back(0);
  long long r = 0;
  M->max_row_nnz = 0;
  while (r < n_rows) {
    const long long base = rp[(size_t)r] & ~1LL;
    long long e = r + 1;
    while (e < n_rows && (e - r) < mgk::MAXROWS && (rp[(size_t)e + 1] - base) <= mgk::CHUNK) ++e;
    blk.push_back((int)e);
    r = e;
  }
  for (long long i = 0; i < n_rows; ++i) M->max_row_nnz = (int)std::min<long long>(0x7fffffff, std::max<long long>(M->max_row_nnz, rp[(size_t)i + 1] - rp[(size_t)i]));
  M->rows_sorted = true;
  for (long long i = 0; i < n_rows && M->rows_sorted; ++i)
    for (long long k = rp[(size_t)i] + 1; k < rp[(size_t)i + 1] && M->rows_sorted; ++k)
      if (rowval[k] < rowval[k - 1]) M->rows_sorted = false;
  M->nblocks = (int)blk.size() - 1;
  M->nblocks_mm = 0;
  MG_TRY(M->rowptr64.alloc(rp.size()));
  MG_TRY(M->blk_row.alloc(blk.size()));
  HIP_TRY(hipMemcpy(M->rowptr64.p, rp.data(), rp.size() * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->blk_row.p, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
  M->h_blk_row = blk;
  M->set = true;
  M->nt = (12.0 * (double)nnz > 128.0e6);
  if (M->opt.nt >= 0) M->nt = (M->opt.nt == 1);
  if (M->opt.debug_format) std::fprintf(stderr, "[mgvcycle] operator %lld x %lld, nnz %lld: 64-bit row pointers (streaming kernels only)\n", n_rows, n_cols, nnz);
  return MG_OK;
}

// Validate Julia's (colptr,rowval,nzval) of the transposed CSC (1-based Int64), convert to 0-based int32
// CSR (the reference's C side does the -1 per access, parRelax.h:24-27), cut the rows into row blocks
// and upload.
int upload_csr(Csr* M, const Options& opt, long long n_rows, long long n_cols, const long long* colptr,
               const long long* rowval, const double* nzval, long long regular_cols = -1, long long regular_rows = -1) {
  if (n_rows < 1 || n_cols < 1 || !colptr || !rowval || !nzval)
    return fail(MG_ERR_INVALID, "empty operator or null array");
  if (n_rows >= (1LL << 31) - 1 || n_cols >= (1LL << 31) - 1)
    return fail(MG_ERR_UNSUPPORTED, "dimension exceeds int32 device indices");
  if (colptr[0] != 1) return fail(MG_ERR_INVALID, "colptr[1] must be 1 (1-based Julia arrays expected)");
  const long long nnz = colptr[n_rows] - 1;
  if (nnz < 0) return fail(MG_ERR_INVALID, "colptr is not a 1-based pointer array");
  if (nnz >= (1LL << 31) - 4096 || opt.force_rowptr64) {
    if (regular_cols >= 0) return fail(MG_ERR_UNSUPPORTED, "nnz=%lld: box / grid forms of a sharded level hold int32 row pointers", nnz);
    return upload_csr_wide(M, opt, n_rows, n_cols, colptr, rowval, nzval, nnz);
  }
  std::vector<int> rp((size_t)n_rows + 1);
  for (long long i = 0; i <= n_rows; ++i) {
    const long long v = colptr[i] - 1;
    if (v < 0 || v > nnz || (i > 0 && v < (long long)rp[(size_t)i - 1]))
      return fail(MG_ERR_INVALID, "colptr is not a monotone 1-based pointer array at %lld", i);
    rp[(size_t)i] = (int)v;
  }
  const size_t pad = 2 * mgk::BLK;  // loads of a trailing (idx, idx+1) pair stay in bounds
  std::vector<int> ci((size_t)nnz + pad, 0);
  for (long long k = 0; k < nnz; ++k) {
    const long long c = rowval[k] - 1;
    if (c < 0 || c >= n_cols) return fail(MG_ERR_INVALID, "rowval[%lld]=%lld outside 1..%lld", k + 1, rowval[k], n_cols);
    ci[(size_t)k] = (int)c;
  }
  // row blocks: consecutive rows, <= maxrows rows and an (even-aligned) nnz span <= chunk
  // (a box-form local operator computes its owned rows only: the empty halo rows behind them get no row block)
  const long long n_rows_blk = regular_cols >= 0 ? (regular_rows >= 0 ? regular_rows : std::min(regular_cols, n_rows)) : n_rows;
  auto make_blocks = [&](int maxrows, int chunk) {
    std::vector<int> bl;
    bl.push_back(0);
    long long r = 0;
    while (r < n_rows_blk) {
      const long long base = rp[(size_t)r] & ~1LL;
      long long e = r + 1;  // a block always holds at least one row (a longer row takes the long-row path)
      while (e < n_rows_blk && (e - r) < maxrows && (rp[(size_t)e + 1] - base) <= chunk) ++e;
      bl.push_back((int)e);
      r = e;
    }
    return bl;
  };
  std::vector<int> blk = make_blocks(mgk::MAXROWS, mgk::CHUNK);
  std::vector<int> blk_mm = make_blocks(mgk::MM_MAXROWS, mgk::MM_CHUNK);
  M->release();
  M->opt = opt;
  M->regular_cols = regular_cols;
  M->regular_rows = regular_rows;
  M->n_rows = n_rows;
  M->n_cols = n_cols;
  M->nnz = nnz;
  M->nblocks = (int)blk.size() - 1;
  MG_TRY(M->rowptr.alloc(rp.size()));
  MG_TRY(M->colidx.alloc(ci.size()));
  MG_TRY(M->val.alloc((size_t)nnz + pad));
  MG_TRY(M->blk_row.alloc(blk.size()));
  HIP_TRY(hipMemcpy(M->rowptr.p, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->colidx.p, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(M->val.p, 0, ((size_t)nnz + pad) * sizeof(double)));
  HIP_TRY(hipMemcpy(M->val.p, nzval, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->blk_row.p, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
  M->h_blk_row = blk;
  M->max_row_nnz = 0;
  M->rows_sorted = true;
  for (long long i = 0; i < n_rows; ++i) {
    M->max_row_nnz = std::max(M->max_row_nnz, rp[(size_t)i + 1] - rp[(size_t)i]);
    for (int k = rp[(size_t)i] + 1; k < rp[(size_t)i + 1] && M->rows_sorted; ++k)
      if (ci[(size_t)k] < ci[(size_t)k - 1]) M->rows_sorted = false;
  }
  M->nblocks_mm = (int)blk_mm.size() - 1;
  MG_TRY(M->blk_row_mm.alloc(blk_mm.size()));
  HIP_TRY(hipMemcpy(M->blk_row_mm.p, blk_mm.data(), blk_mm.size() * sizeof(int), hipMemcpyHostToDevice));
  M->h_blk_row_mm = blk_mm;
  M->set = true;
  // cache policy of the matrix stream: non-temporal once the operator is too large to stay in the
  // 256 MiB Infinity Cache between two uses anyway (measured, profiles/r01_nt_ab.md: +2..17 % on the
  // 685 MB..1.4 GB operators of C2, -5..25 % on the 89 MB ones); MG_NT=0/1 forces one policy
  M->nt = (12.0 * (double)nnz > 128.0e6);
  if (M->opt.nt >= 0) M->nt = (M->opt.nt == 1);
  if (!M->opt.no_rowclass) {  // few distinct rows (offsets AND values): no matrix stream at all at nrhs == 1
    MG_TRY(build_rowclasses(M, rp.data(), ci.data(), nzval));
    if (M->has_rc) {
      M->h_rp = rp;
      M->h_ci = ci;
    }
  }
  {  // pattern-code the column indices when the operator has few distinct row patterns (grid operators)
    if (!M->opt.no_pattern) MG_TRY(build_patterns(M, rp, ci));
  }
  // long rows (csr_longrow_spmv): 16-bit column indices relative to the row's first column where every row spans < 65536 columns -
  // the matrix stream is 10 instead of 12 bytes per non-zero (the Galerkin levels of an SA-AMG hierarchy: neighbourhoods in a few planes)
  M->has_ci16 = false;
  if (M->longrow() && !M->opt.no_ci16 && nnz > 0) {
    bool fits = true;
    for (long long i = 0; i < n_rows && fits; ++i) {
      const int a = rp[(size_t)i], b = rp[(size_t)i + 1];
      if (b > a && ci[(size_t)b - 1] - ci[(size_t)a] > 65535) fits = false;      // (columns ascending within a row)
      for (int k = a + 1; k < b && fits; ++k)
        if (ci[(size_t)k] < ci[(size_t)k - 1]) fits = false;
    }
    if (fits) {
      std::vector<unsigned short> c16((size_t)nnz + 512, 0);
      std::vector<int> rb((size_t)n_rows, 0);
      for (long long i = 0; i < n_rows; ++i) {
        const int a = rp[(size_t)i], b = rp[(size_t)i + 1];
        const int base = b > a ? ci[(size_t)a] : 0;
        rb[(size_t)i] = base;
        for (int k = a; k < b; ++k) c16[(size_t)k] = (unsigned short)(ci[(size_t)k] - base);
      }
      MG_TRY(M->ci16.alloc(c16.size()));
      MG_TRY(M->rowbase.alloc(rb.size()));
      HIP_TRY(hipMemcpy(M->ci16.p, c16.data(), c16.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(M->rowbase.p, rb.data(), rb.size() * sizeof(int), hipMemcpyHostToDevice));
      M->has_ci16 = true;
    }
  }
  if (M->opt.debug_format)
      std::fprintf(stderr, "[mgvcycle] operator %lld x %lld, nnz %lld: row classes %lld (dictionary %lld, exception rows %d, "
                   "implicit first %d, window %d, paired rows %d), patterns %lld\n", M->n_rows, M->n_cols, M->nnz, M->has_rc ? M->rc_ncls : 0,
                   M->has_rc ? M->rc_entries : 0, M->rc_nexc, (int)M->rc_implicit, (int)M->rc_window, (int)M->rc_pair,
                   M->has_pat ? M->npat : 0);
  return MG_OK;
}

// column -> entries in ascending row order (stable counting sort of the stored pattern), for colsumsq_kernel
int build_transposed_pattern(Csr& A) {
  if (A.wide) return fail(MG_ERR_UNSUPPORTED, "operators with 64-bit row pointers are not transposed on the device");
  if (A.has_t) return MG_OK;
  std::vector<int> rp((size_t)A.n_rows + 1), ci((size_t)A.nnz);
  HIP_TRY(hipMemcpy(rp.data(), A.rowptr.p, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (A.nnz > 0) HIP_TRY(hipMemcpy(ci.data(), A.colidx.p, ci.size() * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<int> tp((size_t)A.n_cols + 1, 0), perm((size_t)std::max<long long>(A.nnz, 1));
  for (long long k = 0; k < A.nnz; ++k) ++tp[(size_t)ci[(size_t)k] + 1];
  for (long long j = 0; j < A.n_cols; ++j) tp[(size_t)j + 1] += tp[(size_t)j];
  std::vector<int> next(tp.begin(), tp.end() - 1);
  for (long long i = 0; i < A.n_rows; ++i)
    for (int k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k) perm[(size_t)next[(size_t)ci[(size_t)k]]++] = k;
  MG_TRY(A.t_ptr.alloc(tp.size()));
  MG_TRY(A.t_perm.alloc(perm.size()));
  HIP_TRY(hipMemcpy(A.t_ptr.p, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(A.t_perm.p, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
  A.has_t = true;
  return MG_OK;
}

Csr* pick(mg_hierarchy* h, long long level, long long which) {
  if (level < 1 || level > h->nlevels) return nullptr;
  Level& L = h->lev[level - 1];
  if (which == MG_OP_A) return &L.A;
  if (which == MG_OP_P) return &L.P;
  if (which == MG_OP_R) return &L.R;
  return nullptr;
}


// ---- sparse triangular factors in parLU's layout (mg_set_coarse_lu_FP64_INT64 / _CF64_INT64) -------------------------
// Dependency levels of the rows [0, n-M) of a triangular factor; the trailing M rows are handled apart (for U they
// are solved BEFORE every level, for L after all of them), so they impose no ordering here.
void lu_levels(long long n, const std::vector<int>& P, const std::vector<int>& Cc, bool lower, int M, std::vector<int>& order,
               std::vector<int>& lvlptr) {
  const int na = (int)n - M;
  std::vector<int> lvl((size_t)na, 0);
  int nl = 0;
  if (lower) {
    for (int i = 0; i < na; ++i) {
      int m = 0;
      for (int k = P[(size_t)i]; k < P[(size_t)i + 1] - 1; ++k) m = std::max(m, lvl[(size_t)Cc[(size_t)k]] + 1);
      lvl[(size_t)i] = m;
      nl = std::max(nl, m + 1);
    }
  } else {
    for (int i = na - 1; i >= 0; --i) {
      int m = 0;
      for (int k = P[(size_t)i] + 1; k < P[(size_t)i + 1]; ++k)
        if (Cc[(size_t)k] < na) m = std::max(m, lvl[(size_t)Cc[(size_t)k]] + 1);
      lvl[(size_t)i] = m;
      nl = std::max(nl, m + 1);
    }
  }
  lvlptr.assign((size_t)nl + 1, 0);
  for (int i = 0; i < na; ++i) lvlptr[(size_t)lvl[(size_t)i] + 1]++;
  for (int l = 0; l < nl; ++l) lvlptr[(size_t)l + 1] += lvlptr[(size_t)l];
  order.resize((size_t)na);
  std::vector<int> pos(lvlptr.begin(), lvlptr.end() - 1);
  for (int i = 0; i < na; ++i) order[(size_t)pos[(size_t)lvl[(size_t)i]]++] = i;
}

// 1-based Int64 CSR factor -> 0-based int32 arrays, checked (L: diagonal last, U: diagonal first), and its levels.
int lu_convert(long long n, const long long* ptr, const long long* col, bool lower, std::vector<int>& P, std::vector<int>& Cc,
               std::vector<int>& order, std::vector<int>& lvlptr) {
  const size_t N = (size_t)n;
  const long long nnz = ptr[n] - 1;
  P.resize(N + 1);
  Cc.resize((size_t)nnz);
  for (size_t i = 0; i <= N; ++i) P[i] = (int)(ptr[i] - 1);
  for (long long k = 0; k < nnz; ++k) {
    const long long c = col[k] - 1;
    if (c < 0 || c >= n) return fail(MG_ERR_INVALID, "factor column index out of range");
    Cc[(size_t)k] = (int)c;
  }
  if (lower) {
    for (size_t i = 0; i < N; ++i) {
      if (P[i + 1] - P[i] < 1 || Cc[(size_t)P[i + 1] - 1] != (int)i) return fail(MG_ERR_INVALID, "L: the diagonal must be the last entry of row %zu", i + 1);
      for (int k = P[i]; k < P[i + 1] - 1; ++k)
        if (Cc[(size_t)k] >= (int)i) return fail(MG_ERR_INVALID, "L is not lower triangular");
    }
  } else {
    for (size_t ii = 0; ii < N; ++ii) {
      if (P[ii + 1] - P[ii] < 1 || Cc[(size_t)P[ii]] != (int)ii) return fail(MG_ERR_INVALID, "U: the diagonal must be the first entry of row %zu", ii + 1);
      for (int k = P[ii] + 1; k < P[ii + 1]; ++k)
        if (Cc[(size_t)k] <= (int)ii) return fail(MG_ERR_INVALID, "U is not upper triangular");
    }
  }
  lu_levels(n, P, Cc, lower, 0, order, lvlptr);
  return MG_OK;
}

}  // namespace
