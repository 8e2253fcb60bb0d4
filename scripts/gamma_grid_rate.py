"""Constrained GASS updates with the gamma-grid likelihood (rng="device"), two configurations:
  A  one W+V update at (512,256,64), R = 4, K = 5, gass_ngrid 100, G = 20, against the plain Poisson (identity link)
     update of the same shape and constraints, measured in the same run;
  B  a dose-response-like shape (1024,256,9), R = 6, K = 5, tf_order 2, G = 20, with and without ep_approx.
Every line: wall ms per W+V update and the ms of the BTF_K_ESS kernels.  python scripts/gamma_grid_rate.py [A|B]"""
import contextlib, io, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
from functionalmf_amd.likelihoods import GammaGridLikelihood
from functionalmf_amd import utils


def problem(N, M, T, R, K, G, seed=1, upper=True):
    rs = np.random.RandomState(seed)
    W = rs.gamma(2.0, 0.5, size=(N, K)); W[np.triu_indices(K, 1)] = 0
    V = np.zeros((M, T, K))
    V[:, -1] = rs.gamma(2.0, 0.2, size=(M, K))
    for t in range(T - 2, -1, -1):
        V[:, t] = V[:, t + 1] + rs.gamma(1.0, 0.2, size=(M, K)) * (rs.rand(M, 1) < 0.3)
    W *= 0.95 / np.einsum("nk,mtk->nmt", W, V).max()
    lik = GammaGridLikelihood(np.linspace(0.6, 1.4, G), np.full(G, 1.0 / G), 0.03)
    eta = np.einsum("nk,mtk->nmt", W, V)
    comp = rs.choice(G, size=eta.shape)
    Y = rs.gamma(lik.shape_grid[comp][..., None], (lik.scale_grid[comp] * eta)[..., None], size=eta.shape + (R,))
    C_zero = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
    C_mono = np.array([np.concatenate([np.zeros(i), [1, -1], np.zeros(T - i - 2), [-1e-2]]) for i in range(T - 1)])
    C_one = np.concatenate([np.eye(T) * -1, np.full((T, 1), -1)], axis=1)
    return W, V, Y, lik, np.concatenate([C_zero, C_one, C_mono] if upper else [C_zero, C_mono], axis=0)


def rate(m, Y, n=10):
    for _ in range(2):
        m._resample_W(Y)
        m._resample_V(Y)
    m.sync()
    m._ctx.call("btf_set_profiling", 1)
    m._ctx.kernel_times()
    t0 = time.perf_counter()
    for _ in range(n):
        m._resample_W(Y)
        m._resample_V(Y)
    m.sync()
    return 1e3 * (time.perf_counter() - t0) / n, m._ctx.kernel_times()["ess"][0] / n


def make(N, M, T, K, tf, W, V, Cons, lik, ll, ep=None):
    np.random.seed(2)                     # (the starting hyper-parameters come from the legacy generator)
    return ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, ll, Cons, likelihood_param=lik if ll == "gamma_grid" else None,
                                                          ep_approx=ep, gass_ngrid=100, nembeds=K, tf_order=tf, sigma2_init=1.0,
                                                          lam2_init=0.5, W_init=W, V_init=V, rng="device", device_seed=1)


which = sys.argv[1] if len(sys.argv) > 1 else "AB"
if "A" in which:
    N, M, T, R, K, G = 512, 256, 64, 4, 5, 20
    # positivity and monotonicity (127 rows, as scripts/gass_rate.py): with fit.py's tau <= 1 rows too (191 at T = 64) the
    # constraint matrix does not fit the column analysis's LDS at this depth
    W, V, Y, lik, Cons = problem(N, M, T, R, K, G, upper=False)
    res = {"config": "A", "shape": [N, M, T, R, K], "G": G, "ngrid": 100, "constraints": int(Cons.shape[0])}
    res["gamma_grid_ms"], res["gamma_grid_kernel_ms"] = rate(make(N, M, T, K, 0, W, V, Cons, lik, "gamma_grid"), Y)
    Yp = np.random.RandomState(3).poisson(np.repeat(np.einsum("nk,mtk->nmt", W, V)[..., None] * 20, R, axis=-1)).astype(float)
    # the Poisson identity-link update of the same shape and constraints
    res["poisson_identity_ms"], res["poisson_identity_kernel_ms"] = rate(make(N, M, T, K, 0, W, V, Cons, None, "poisson_identity"), Yp)
    print(json.dumps(res), flush=True)
if "B" in which:
    N, M, T, R, K, G = 1024, 256, 9, 6, 5, 20
    W, V, Y, lik, Cons = problem(N, M, T, R, K, G, seed=2)
    with contextlib.redirect_stdout(io.StringIO()):
        ep = utils.ep_from_mf(Y, W, V, mode="multiplier", multiplier=3)
    res = {"config": "B", "shape": [N, M, T, R, K], "G": G, "ngrid": 100, "tf_order": 2, "constraints": int(Cons.shape[0])}
    res["plain_ms"], res["plain_kernel_ms"] = rate(make(N, M, T, K, 2, W, V, Cons, lik, "gamma_grid"), Y)
    res["ep_ms"], res["ep_kernel_ms"] = rate(make(N, M, T, K, 2, W, V, Cons, lik, "gamma_grid", ep), Y)
    print(json.dumps(res), flush=True)
