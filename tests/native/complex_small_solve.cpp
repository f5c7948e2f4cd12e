// The k x k solve of the block drivers (SmallMatT<S>, sm_solve, sm_mul, sm_scaled_identity of csrc/mg_krylov_host.hpp) for
// S = std::complex<double>, on its own: reads cases from the file named on the command line, prints one line per case.  Built and
// run by tests/test_complex_block_host.py with the host sanitizers; includes nothing of the library but that header.
//   solve_cx k nc  A (k*k pairs, row-major)  B (k*nc pairs)   ->  singular-flag, X = A \ B (k*nc pairs)
//   solve_re k nc  A (k*k)  B (k*nc)                           ->  singular-flag, X (the double instantiation, as pairs with zero imaginary part)
//   ident_cx k re im  M (k*k pairs)                            ->  M * (v I) (k*k pairs)
#include <complex>
#include <cstdio>
#include <fstream>
#include <string>

#include "../../multigrid.jl_amd/csrc/mg_krylov_host.hpp"

typedef std::complex<double> zc;

static void get(std::istream& in, double& v) { in >> v; }
static void get(std::istream& in, zc& v) {
  double a = 0.0, b = 0.0;
  in >> a >> b;
  v = zc(a, b);
}
static void put(double v) { std::printf(" %.17g 0", v); }
static void put(const zc& v) { std::printf(" %.17g %.17g", v.real(), v.imag()); }

template <class S>
static SmallMatT<S> get_mat(std::istream& in, int r, int c) {
  SmallMatT<S> M(r, c);
  for (S& v : M.a) get(in, v);
  return M;
}

template <class S>
static void solve(std::istream& in) {
  int k = 0, nc = 0;
  in >> k >> nc;
  const SmallMatT<S> A = get_mat<S>(in, k, k), B = get_mat<S>(in, k, nc);
  SmallMatT<S> X;
  const bool ok = sm_solve(A, B, X);
  std::printf(" %d", ok ? 0 : 1);
  if (ok)
    for (const S& v : X.a) put(v);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string cmd;
  while (in >> cmd) {
    std::printf("%s", cmd.c_str());
    if (cmd == "solve_cx") {
      solve<zc>(in);
    } else if (cmd == "solve_re") {
      solve<double>(in);
    } else if (cmd == "ident_cx") {
      int k = 0;
      zc v;
      in >> k;
      get(in, v);
      const SmallMatT<zc> M = get_mat<zc>(in, k, k);
      const SmallMatT<zc> P = sm_mul(M, sm_scaled_identity(k, v));
      for (const zc& e : P.a) put(e);
    } else {
      return 3;
    }
    std::printf("\n");
    if (!in) return 5;
  }
  return 0;
}
