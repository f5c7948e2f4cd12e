// Stand-alone driver of the replay of a complex hierarchy's GMRES coarsest solve in csrc/mg_krylov_host.hpp (coarse_gmres_replay on
// HessenbergLsq<std::complex<double>>) for tests/test_complex_coarse_gmres_host.py: reads cases from the file named on the command
// line (white-space separated tokens), prints one line of results per case with 17 significant digits.  Built by the test with
// -fsanitize=address,undefined; it includes nothing else of the library.
//   replay m tol    the table of (m + 1)^2 doubles: ||b||^2, then per step i: h_0 .. h_i (re im each), ||w||^2
//                   -> "used flag resvec (used) y (used pairs)"
#include "../../multigrid.jl_amd/csrc/mg_krylov_host.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

typedef std::complex<double> zc;

static void put(double v) { std::printf(" %.17g", v); }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string cmd;
  while (in >> cmd) {
    std::printf("%s", cmd.c_str());
    if (cmd == "replay") {
      int m = 0;
      double tol = 0.0;
      in >> m >> tol;
      if (m < 1 || m > 64) return 3;
      std::vector<double> tab((size_t)(m + 1) * (m + 1));
      for (double& v : tab) in >> v;
      if (coarse_gmres_slot(m) != (int)tab.size()) return 3;
      HessenbergLsq<zc> Q(m);
      std::vector<double> resvec((size_t)m, 0.0);
      int used = 0;
      long long flag = 0;
      coarse_gmres_replay(tab.data(), tol, Q, used, flag, resvec.data());
      std::printf(" %d %lld", used, flag);
      for (int i = 0; i < used; ++i) put(resvec[(size_t)i]);
      for (int i = 0; i < used; ++i) {
        put(Q.y[(size_t)i].real());
        put(Q.y[(size_t)i].imag());
      }
    } else {
      return 4;
    }
    std::printf("\n");
    if (!in) return 5;
  }
  return 0;
}
