// The small complex algebra of the complex block FGMRES driver (sm_chol_semidefinite, sm_tri_pinv, sm_lstsq and sm_mul of
// csrc/mg_krylov_host.hpp on SmallMatT<std::complex<double>>), on its own: reads cases from the file named on the command line, prints
// one line per case.  Built and run by tests/test_complex_block_fgmres_host.py with the host sanitizers; includes nothing of the
// library but that header.  Matrices are row-major (re, im) pairs.
//   chol_cx k  G (k*k)                 ->  Rf (k*k), upper triangular with G = Rf^H Rf; dropped pivots give zero rows
//   tripinv_cx k  R (k*k)              ->  T (k*k) with W T = W R^+
//   lstsq_cx m n k  H (m*n)  xi (m*k)  ->  ||xi - H Y||_F 0, Y (n*k)
//   chol_re k  G (k*k reals)           ->  the double form's Rf, as pairs with zero imaginary part
#include <complex>
#include <cstdio>
#include <fstream>
#include <string>

#include "../../multigrid.jl_amd/csrc/mg_krylov_host.hpp"

typedef std::complex<double> zc;

static SmallMatC get_mat(std::istream& in, int r, int c) {
  SmallMatC M(r, c);
  for (zc& v : M.a) {
    double a = 0.0, b = 0.0;
    in >> a >> b;
    v = zc(a, b);
  }
  return M;
}
static void put(const SmallMatC& M) {
  for (const zc& v : M.a) std::printf(" %.17g %.17g", v.real(), v.imag());
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string cmd;
  while (in >> cmd) {
    std::printf("%s", cmd.c_str());
    if (cmd == "chol_cx") {
      int k = 0;
      in >> k;
      put(sm_chol_semidefinite(get_mat(in, k, k)));
    } else if (cmd == "tripinv_cx") {
      int k = 0;
      in >> k;
      put(sm_tri_pinv(get_mat(in, k, k)));
    } else if (cmd == "lstsq_cx") {
      int m = 0, n = 0, k = 0;
      in >> m >> n >> k;
      const SmallMatC H = get_mat(in, m, n), xi = get_mat(in, m, k);
      SmallMatC Y;
      const double res = sm_lstsq(H, xi, Y);
      std::printf(" %.17g 0", res);
      put(Y);
    } else if (cmd == "chol_re") {
      int k = 0;
      in >> k;
      SmallMat G(k, k);
      for (double& v : G.a) in >> v;
      const SmallMat R = sm_chol_semidefinite(G);
      for (double v : R.a) std::printf(" %.17g 0", v);
    } else {
      return 3;
    }
    std::printf("\n");
    if (!in) return 5;
  }
  return 0;
}
