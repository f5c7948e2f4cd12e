// Stand-alone driver of the FGMRES relaxation's small least squares in csrc/mg_krylov_host.hpp (RelaxLsqC, and RelaxLsq beside it) for
// tests/test_complex_kcycle_host.py: reads cases from the file named on the command line (white-space separated tokens), prints one
// line of results per case with 17 significant digits.  Built by the test with -fsanitize=address,undefined; it includes nothing else
// of the library.
//   relax_cx k m rnorm0    H (k*k (re im) pairs, row-major; the upper triangle of the leading m x m block is used), xi (m pairs)
//                          -> "t (k pairs) rn": the capacity is k, the solve is on the leading m x m block
//   relax_real k rnorm0    H (k*k, row-major; the upper triangle is used), xi (k)   -> "t (k) rn"   (the real RelaxLsq)
#include "../../multigrid.jl_amd/csrc/mg_krylov_host.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

typedef std::complex<double> zc;

static void put(double v) { std::printf(" %.17g", v); }
static zc get_c(std::istream& in) {
  double a = 0.0, b = 0.0;
  in >> a >> b;
  return zc(a, b);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string cmd;
  while (in >> cmd) {
    std::printf("%s", cmd.c_str());
    if (cmd == "relax_cx") {
      int k = 0, m = 0;
      double rnorm0 = 0.0;
      in >> k >> m >> rnorm0;
      if (k < 1 || m < 1 || m > k) return 3;
      std::vector<zc> H((size_t)k * k);
      for (zc& v : H) v = get_c(in);
      RelaxLsqC Q(k);
      for (int j = 0; j < m; ++j)
        for (int i = 0; i <= j; ++i) Q.set(i, j, H[(size_t)i * k + j]);
      for (int j = 0; j < m; ++j) Q.xi[(size_t)j] = get_c(in);
      const double rn = Q.step(m, rnorm0);
      for (const zc& v : Q.t()) {
        put(v.real());
        put(v.imag());
      }
      put(rn);
    } else if (cmd == "relax_real") {
      int k = 0;
      double rnorm0 = 0.0;
      in >> k >> rnorm0;
      if (k < 1) return 3;
      std::vector<double> H((size_t)k * k);
      for (double& v : H) in >> v;
      RelaxLsq Q(k);
      for (int j = 0; j < k; ++j)
        for (int i = 0; i <= j; ++i) Q.set(i, j, H[(size_t)i * k + j]);
      for (double& v : Q.xi) in >> v;
      const double rn = Q.step(rnorm0);
      for (double v : Q.t()) put(v);
      put(rn);
    } else {
      return 4;
    }
    std::printf("\n");
    if (!in) return 5;
  }
  return 0;
}
