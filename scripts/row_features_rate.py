"""Binary row features in the constrained model (rng="device"): the W step with the Bernoulli side term and the derived
constraints against the W step without features IN THE SAME RUN, the U step alone, and the accepted share of one
host-driven update each.  Two shapes, F = 32 and F = 1024 features each:
  D  the dose-response shape (1024,256,9), R = 6, K = 5, tf_order 2, the 26 constraints of doseresponse/fit.py:58-61,
     gamma_grid (G = 20), EP-centred;
  P  (512,256,64), R = 4, K = 5, poisson_identity, positivity and monotonicity.
Host wall clock around n synchronised steps after a warm-up, median of 5 repeats; beside it the ms of the BTF_K_ESS
kernels per step.  python scripts/row_features_rate.py [D|P] [--timing-only]"""
import contextlib, io, json, os, sys, time
TIMING_ONLY = "--timing-only" in sys.argv
sys.argv = [a for a in sys.argv if a != "--timing-only"]
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
from functionalmf_amd import utils
from functionalmf_amd.likelihoods import GammaGridLikelihood


def problem(N, M, T, R, K, G, seed=1, upper=True):
    """The simulated curves, gamma-grid likelihood and constraints of scripts/gamma_grid_rate.py."""
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


def features(W, F, seed):
    rs = np.random.RandomState(seed)
    U = rs.uniform(0.05, 1.0, (F, W.shape[1])) / (1.25 * W.sum(axis=1).max())
    P = W @ U.T
    X = (rs.rand(W.shape[0], F) < P / P.max() * 0.8 + 0.1).astype(float)
    X[rs.rand(*X.shape) < 0.1] = np.nan
    return X, U


def timed(step, sync, n=10, warm=3, reps=5):
    for _ in range(warm):
        step()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        sync()
        out.append(1e3 * (time.perf_counter() - t0) / n)
    return float(np.median(out))


def kernel_ms(m, step, n=5):
    m.sync()
    m._ctx.call("btf_set_profiling", 1)
    m._ctx.kernel_times()
    for _ in range(n):
        step()
    m.sync()
    ms = m._ctx.kernel_times()["ess"][0] / n
    m._ctx.call("btf_set_profiling", 0)
    return ms


def run(tag, dims, ll, lik, tf, W, V, Y, Cons, ep):
    N, M, T, K = dims

    def make(rng, X=None, U=None):
        np.random.seed(2)
        return ConstrainedNonconjugateBayesianTensorFiltering(
            N, M, T, ll, Cons, likelihood_param=lik, ep_approx=ep, gass_ngrid=100, nembeds=K, tf_order=tf, sigma2_init=1.0,
            lam2_init=0.5, W_init=W, V_init=V, rng=rng, device_seed=1, row_features=X, feature_embeddings=U)
    plain = make("device")
    w_plain = timed(lambda: plain._resample_W(Y), plain.sync)
    wk_plain = kernel_ms(plain, lambda: plain._resample_W(Y))
    for F in (32, 1024):
        X, U = features(W, F, 5)
        m = make("device", X, U)
        res = {"shape": tag, "dims": [N, M, T, K], "likelihood": ll, "ep": ep is not None, "constraints": int(Cons.shape[0]),
               "ngrid": 100, "F": F, "w_plain_ms": w_plain, "w_plain_kernel_ms": wk_plain}
        res["w_features_ms"] = timed(lambda: m._resample_W(Y), m.sync)
        res["w_features_kernel_ms"] = kernel_ms(m, lambda: m._resample_W(Y))
        res["w_ratio"] = res["w_features_ms"] / w_plain
        res["u_ms"] = timed(lambda: m._resample_U(), m.sync)
        res["u_kernel_ms"] = kernel_ms(m, lambda: m._resample_U())
        if not TIMING_ONLY:
            h = make("host", X, U)
            h._resample_W(Y)
            res["accepted_w"] = float(np.sum(h.gass_info["accepted"]) / max(1, np.sum(h.gass_info["candidates"])))
            h._resample_U()
            res["accepted_u"] = float(np.sum(h.gass_info["accepted"]) / max(1, np.sum(h.gass_info["candidates"])))
        print(json.dumps(res), flush=True)


which = sys.argv[1] if len(sys.argv) > 1 else "DP"
if "D" in which:
    N, M, T, R, K, G = 1024, 256, 9, 6, 5, 20
    W, V, Y, lik, Cons = problem(N, M, T, R, K, G, seed=2)
    with contextlib.redirect_stdout(io.StringIO()):
        ep = utils.ep_from_mf(Y, W, V, mode="multiplier", multiplier=3)
    run("doseresponse", (N, M, T, K), "gamma_grid", lik, 2, W, V, Y, Cons, ep)
if "P" in which:
    N, M, T, R, K = 512, 256, 64, 4, 5
    W, V, _, _, Cons = problem(N, M, T, R, K, 20, upper=False)
    Y = np.random.RandomState(3).poisson(np.repeat(np.einsum("nk,mtk->nmt", W, V)[..., None] * 20, R, axis=-1)).astype(float)
    run("poisson", (N, M, T, K), "poisson_identity", None, 0, W, V, Y, Cons, None)
