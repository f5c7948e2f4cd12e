// Stand-alone driver of csrc/mg_krylov_host.hpp for tests/test_krylov_host_algebra.py: reads cases from the file named on the command
// line (white-space separated tokens), prints one line of results per case with 17 significant digits.  Built by the test with
// -fsanitize=address,undefined; it includes nothing else of the library.
//   hess_real m beta solve   then per column i: h_0 .. h_i, h_{i+1,i}           -> per column "est c_re c_im s", then (solve = 1) "y ..."
//   hess_cx   m beta solve   the same with (re im) pairs for h_0 .. h_i
//   relax k rnorm0           H (k*k, row-major; the upper triangle is used), xi -> "t ... rn"
//   solve k nc               A (k*k), B (k*nc)                                  -> X
//   lstsq m n k              H (m*n), xi (m*k)                                  -> Y (n*k), residual norm
//   cholpinv k               G (k*k)                                            -> R (k*k), T (k*k)
//   report n                 n values                                           -> what KrylovReport wrote, with and without pointers
#include "../../multigrid.jl_amd/csrc/mg_krylov_host.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

typedef std::complex<double> zc;

static void put(double v) { std::printf(" %.17g", v); }
static void put(const zc& v) { std::printf(" %.17g %.17g", v.real(), v.imag()); }
static double re(double v) { return v; }
static double re(const zc& v) { return v.real(); }
static double im(double) { return 0.0; }
static double im(const zc& v) { return v.imag(); }
static void get(std::istream& in, double& v) { in >> v; }
static void get(std::istream& in, zc& v) {
  double a = 0.0, b = 0.0;
  in >> a >> b;
  v = zc(a, b);
}
static SmallMat get_mat(std::istream& in, int r, int c) {
  SmallMat M(r, c);
  for (double& v : M.a) in >> v;
  return M;
}
static void put_mat(const SmallMat& M) {
  for (double v : M.a) put(v);
}

template <class S>
static void hess(std::istream& in) {
  int m = 0, solve = 0;
  double beta = 0.0;
  in >> m >> beta >> solve;
  HessenbergLsq<S> G(m);
  G.begin(beta);
  for (int i = 0; i < m; ++i) {
    for (int k = 0; k <= i; ++k) get(in, G.h(k, i));
    in >> G.hsub(i);
    const double est = G.close_column(i);
    put(est);
    put(re(G.cs[(size_t)i]));
    put(im(G.cs[(size_t)i]));
    put(G.sn[(size_t)i]);
  }
  if (solve)
    for (const S& v : G.solve(m)) put(v);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string cmd;
  while (in >> cmd) {
    std::printf("%s", cmd.c_str());
    if (cmd == "hess_real") {
      hess<double>(in);
    } else if (cmd == "hess_cx") {
      hess<zc>(in);
    } else if (cmd == "relax") {
      int k = 0;
      double rnorm0 = 0.0;
      in >> k >> rnorm0;
      const SmallMat H = get_mat(in, k, k);
      RelaxLsq Q(k);
      for (int j = 0; j < k; ++j)
        for (int i = 0; i <= j; ++i) Q.set(i, j, H(i, j));
      for (double& v : Q.xi) in >> v;
      const double rn = Q.step(rnorm0);
      for (double v : Q.t()) put(v);
      put(rn);
    } else if (cmd == "solve") {
      int k = 0, nc = 0;
      in >> k >> nc;
      const SmallMat A = get_mat(in, k, k), B = get_mat(in, k, nc);
      SmallMat X;
      if (!sm_solve(A, B, X)) return 3;
      put_mat(X);
    } else if (cmd == "lstsq") {
      int m = 0, n = 0, k = 0;
      in >> m >> n >> k;
      const SmallMat H = get_mat(in, m, n), xi = get_mat(in, m, k);
      SmallMat Y;
      const double res = sm_lstsq(H, xi, Y);
      put_mat(Y);
      put(res);
    } else if (cmd == "cholpinv") {
      int k = 0;
      in >> k;
      const SmallMat R = sm_chol_semidefinite(get_mat(in, k, k));
      put_mat(R);
      put_mat(sm_tri_pinv(R));
    } else if (cmd == "report") {
      int n = 0;
      in >> n;
      std::vector<double> vals((size_t)n), resvec((size_t)n + 1, -1.0);
      for (double& v : vals) in >> v;
      KrylovReport none(nullptr, nullptr, nullptr, nullptr);
      for (double v : vals) none.record(v);
      none.set(0, 7.0);
      put((double)none.finish(5, -3));
      put((double)none.nr);
      long long iters = -7, flag = -7, nres = -7;
      KrylovReport rep(&iters, &flag, resvec.data(), &nres);
      for (double v : vals) rep.record(v);
      rep.set(0, 7.0);
      put((double)rep.finish(5, -3));
      put((double)iters);
      put((double)flag);
      put((double)nres);
      for (double v : resvec) put(v);
    } else {
      return 4;
    }
    std::printf("\n");
    if (!in) return 5;
  }
  return 0;
}
