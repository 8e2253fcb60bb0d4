"""EP-centred against plain GASS updates at one size, measured in the same run (rng="device"), plus the accepted-candidate
fraction of one host-driven update each.  python scripts/gass_ep_rate.py [N M T K ngrid] [--timing-only]"""
import contextlib, io, json, os, sys, time
TIMING_ONLY = "--timing-only" in sys.argv
sys.argv = [a for a in sys.argv if a != "--timing-only"]
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from functionalmf_amd.factor import ConstrainedNonconjugateBayesianTensorFiltering
from functionalmf_amd import utils

N, M, T, K, ngrid = [int(a) for a in sys.argv[1:6]] if len(sys.argv) >= 6 else (512, 256, 64, 5, 100)
rs = np.random.RandomState(1)
Wt = rs.gamma(2.0, 0.5, size=(N, K)); Wt[np.triu_indices(K, 1)] = 0
Vt = np.zeros((M, T, K))
for j in range(M):
    Vt[j, -1] = rs.gamma(2.0, 0.5, size=K)
    for t in range(T - 2, -1, -1):
        Vt[j, t] = Vt[j, t + 1] + (rs.gamma(1.0, 0.6, size=K) if rs.rand() < 0.3 else 0.0)
Y = rs.poisson(np.einsum("nk,mtk->nmt", Wt, Vt)).astype(float)
Cons = np.concatenate([np.eye(T), np.zeros((T, 1))], axis=1)
mono = np.array([np.concatenate([np.zeros(t), [1, -1], np.zeros(T - t - 2), [-1e-2]]) for t in range(T - 1)])
Cons = np.concatenate([Cons, mono], axis=0)
with contextlib.redirect_stdout(io.StringIO()):
    ep = utils.ep_from_mf(Y, Wt, Vt, mode="multiplier", multiplier=3)


def make(ep_approx, rng):
    np.random.seed(2)
    return ConstrainedNonconjugateBayesianTensorFiltering(N, M, T, "poisson_identity", Cons, ep_approx=ep_approx, gass_ngrid=ngrid,
                                                          nembeds=K, tf_order=0, sigma2_init=1.0, lam2_init=0.5, W_init=Wt,
                                                          V_init=Vt, rng=rng, device_seed=1)


def rate(m, n=10):
    for _ in range(3):
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


def accepted(m):
    out = []
    for what in (0, 1):
        (m._resample_W if what == 0 else m._resample_V)(Y)
        gi = m.gass_info
        out.append(float(np.sum(gi["accepted"]) / max(1, np.sum(gi["candidates"]))))
    return out


res = {"shape": [N, M, T, K], "constraints": int(Cons.shape[0]), "ngrid": ngrid}
res["plain_ms"], res["plain_kernel_ms"] = rate(make(None, "device"))
res["ep_ms"], res["ep_kernel_ms"] = rate(make(ep, "device"))
res["ratio"] = res["ep_ms"] / res["plain_ms"]
if not TIMING_ONLY:
    res["accepted_plain_w_v"] = accepted(make(None, "host"))
    res["accepted_ep_w_v"] = accepted(make(ep, "host"))
print(json.dumps(res))
