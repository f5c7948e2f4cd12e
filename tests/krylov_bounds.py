"""TEST INFRASTRUCTURE ONLY.  The two bounds every kernel-level Krylov test shares (tests/test_dist_krylov.py: the halo form's fused
passes; tests/krylov_pass_cases.py: the real single-GPU drivers' passes): an updated vector against the long-double value of its
expression, a sum against the long-double sum of its terms.  `got` is a torch tensor or a numpy array."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def _ld(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(LD)


def _close_vec(name, got, ref_ld, *terms):
    """|got - ref| <= 2 ulp of the largest magnitude among the expression's terms, partial results and result (every rounding of the
    unfused fp64 evaluation is at most half an ulp of one of them; no pass below has more than four)."""
    mag = np.abs(ref_ld)
    for t in terms:
        mag = np.maximum(mag, np.abs(t))
    err = np.abs(_ld(got) - ref_ld)
    bound = 2.0 * np.spacing(mag.astype(np.float64)).astype(LD)
    worst = float((err / bound).max())
    print(f"    {name}: worst error {2 * worst:.3f} ulp (bound 2)")
    assert worst <= 1.0, (name, worst)
    return worst


def _close_sum(name, got, terms_ld):
    """|got - sum| <= n * 2^-53 * sum|terms| (any order of summation of fp64 products)."""
    ref, bound = terms_ld.sum(), terms_ld.size * LD(U) * np.abs(terms_ld).sum()
    err = abs(LD(got) - ref)
    print(f"    {name}: |sum - reference| = {float(err):.3e} (bound {float(bound):.3e})")
    assert err <= bound, (name, float(err), float(bound))
    return float(err / bound) if bound > 0 else 0.0
