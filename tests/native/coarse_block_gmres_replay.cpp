// Stand-alone driver of the replay of a complex hierarchy's BLOCK GMRES coarsest solve in csrc/mg_krylov_host.hpp
// (coarse_block_gmres_replay on BlockHessenbergLsq) for tests/test_complex_block_coarse_gmres_host.py: reads cases from the file named on
// the command line (white-space separated tokens), prints one line of results per case with 17 significant digits.  Built by the test
// with -fsanitize=address,undefined; it includes nothing else of the library.
//   replay k m tol   the table of coarse_block_table_len(k, m) doubles: ||B||_F^2, a pad, then k x k complex blocks (row-major, re im):
//                    xi_0, and per step j: H_0j .. H_jj, H_{j+1,j}
//                    -> "used flag resvec (used) Y (used k x k pairs, row-major) dres dY": the last two compare every step with
//                    sm_lstsq on the leading blocks (the block FGMRES driver's route): the largest difference of the residual norms
//                    and, at the last step, of Y
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
      int k = 0, m = 0;
      double tol = 0.0;
      in >> k >> m >> tol;
      if (k < 1 || k > 16 || m < 1 || m > 10) return 3;
      std::vector<double> tab(coarse_block_table_len(k, m));
      for (double& v : tab) in >> v;
      BlockHessenbergLsq Q(k, m);
      std::vector<double> resvec((size_t)m, 0.0);
      int used = 0;
      long long flag = 0;
      SmallMatC Y;
      coarse_block_gmres_replay(tab.data(), k, tol, Q, used, flag, resvec.data(), Y);
      std::printf(" %d %lld", used, flag);
      for (int i = 0; i < used; ++i) put(resvec[(size_t)i]);
      for (const zc& y : Y.a) {
        put(y.real());
        put(y.imag());
      }
      // the same least squares by sm_lstsq on the leading blocks
      double dres = 0.0, dY = 0.0;
      if (used > 0) {
        const double bn = std::sqrt(tab[0]);
        const size_t kk = (size_t)k * k;
        auto at = [&](size_t s, int a, int b) { const double* e = tab.data() + 2 + 2 * (s * kk + (size_t)a * k + b); return zc(e[0], e[1]); };
        for (int j = 0; j < used; ++j) {
          SmallMatC Hb((j + 2) * k, (j + 1) * k), xb((j + 2) * k, k), Yf;
          for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) xb(a, b) = at(0, a, b);
          for (int c = 0; c <= j; ++c)
            for (int i = 0; i <= c + 1; ++i)
              for (int a = 0; a < k; ++a)
                for (int b = 0; b < k; ++b) Hb(i * k + a, c * k + b) = at(coarse_block_slot(c) + (size_t)i, a, b);
          const double err = sm_lstsq(Hb, xb, Yf) / bn;
          dres = std::max(dres, std::fabs(err - resvec[(size_t)j]));
          if (j == used - 1)
            for (size_t e = 0; e < Yf.a.size(); ++e) dY = std::max(dY, std::abs(Yf.a[e] - Y.a[e]));
        }
      }
      put(dres);
      put(dY);
    } else {
      return 4;
    }
    std::printf("\n");
    if (!in) return 5;
  }
  return 0;
}
