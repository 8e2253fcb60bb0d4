"""Posterior similarity on the GPU at the edges of its geometry: sample counts across the sort row's padding, entity counts
across the wave and the partner blocks, every nembeds, `over`, `nearest` and the tiling of the stage.  The distances are
held to the definition (functionalmf_amd/similarity.py) with the tolerances of tests/test_gpu_similarity.py, everything
else to numpy applied to the device's own distances; tilings are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from functionalmf_amd import _native, similarity
from functionalmf_amd.utils import posterior_similarity
from test_gpu_similarity import _states, check_summaries

pytestmark = pytest.mark.gpu

Q = (5, 50, 95, 0, 100, 33.3)


def _check_distances(d, Ws, Vs, along, metric, over=None):
    ref = similarity.distances(Ws, Vs, along, metric, over)
    if metric == "rms":
        assert np.abs(d ** 2 - ref ** 2).max() <= 1e-11 * max((ref ** 2).max(), np.finfo(float).tiny)
    else:
        assert np.abs(d - ref).max() <= 1e-12
    E = d.shape[1]
    assert np.array_equal(d, d.transpose(0, 2, 1)) and (d[:, np.arange(E), np.arange(E)] == 0.0).all()


def _no_ties(d):
    E = d.shape[1]
    srt = np.sort(np.where(np.eye(E, dtype=bool), np.inf, d), axis=2)
    return E <= 2 or (np.diff(srt[:, :, :-1], axis=2) > 0).all()


@pytest.mark.parametrize("S,E", [(1, 5), (2, 5), (1000, 6), (1025, 3)])
@pytest.mark.parametrize("along", ["rows", "cols"])
def test_sample_counts(S, E, along):
    """S = 1 (variance nan, as posterior_functionals), 2, 1000, and 1025: past 1024 the sort row pads to 2048."""
    N, M = (E, 2) if along == "rows" else (3, E)
    Ws, Vs = _states(S, N, M, 4, 2, seed=S)
    out = posterior_similarity(Ws, Vs, along=along, q=Q, nearest=(1, 2), pointwise=True)
    d = out["distances"]
    _check_distances(d, Ws, Vs, along, "rms")
    assert _no_ties(d)
    assert np.isnan(out["var"]).all() == (S == 1)
    check_summaries(out, d, Q, (1, 2))


@pytest.mark.parametrize("E", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("along,metric", [("rows", "rms"), ("cols", "cosine"), ("cols", "rms")])
def test_entity_counts(E, along, metric):
    N, M = (E, 3) if along == "rows" else (4, E)
    Ws, Vs = _states(3, N, M, 5, 3, seed=E)
    out = posterior_similarity(Ws, Vs, along=along, metric=metric, q=Q, nearest=(1, 3, 64, 65), pointwise=True)
    d = out["distances"]
    assert d.shape == (3, E, E)
    _check_distances(d, Ws, Vs, along, metric)
    assert _no_ties(d)
    check_summaries(out, d, Q, (1, 3, 64, 65))
    if E == 1:                                                              # nothing to rank: rank 1, certain
        assert out["expected_rank"].tolist() == [[1.0]] and out["rank_var"].tolist() == [[0.0]]
        assert out["p_nearest"][:, 0, 0].tolist() == [1.0] * 4 and out["mean"].tolist() == [[0.0]]
    else:
        assert (np.diag(out["expected_rank"]) == E).all() and (np.diag(out["p_nearest"][0]) == 0).all()


@pytest.mark.parametrize("metric", ["rms", "cosine"])
@pytest.mark.parametrize("nembeds", range(1, 11))
def test_every_nembeds(nembeds, metric):
    """All twenty instantiations of sim_dist_kernel<K, COS> and the ten of sim_metric_kernel<K>, along the columns: several
    depth blocks (T = 9 > 2 SIM_TB) with a short last one, a full wave of entities and a partial one."""
    Ws, Vs = _states(3, 6, 70, 9, nembeds, seed=10 * nembeds)
    out = posterior_similarity(Ws, Vs, along="cols", metric=metric, pointwise=True)
    _check_distances(out["distances"], Ws, Vs, "cols", metric)
    out = posterior_similarity(Ws[:, :5], Vs[:, :3], along="rows", metric=metric, pointwise=True)
    _check_distances(out["distances"], Ws[:, :5], Vs[:, :3], "rows", metric)


@pytest.mark.parametrize("along", ["rows", "cols"])
def test_over(along):
    """One member, all but one, and a permutation of all: the permutation changes the order of the metric's partial sums,
    so it agrees with over=None to the tolerance of the distances, not bit for bit."""
    Ws, Vs = _states(4, 7, 6, 5, 3, seed=21)
    n_members = 6 if along == "rows" else 7
    whole = posterior_similarity(Ws, Vs, along=along, pointwise=True)
    for over in ([n_members - 2], list(range(1, n_members)), list(np.random.RandomState(2).permutation(n_members))):
        for metric in ("rms", "cosine"):
            out = posterior_similarity(Ws, Vs, along=along, metric=metric, over=over, q=Q, pointwise=True)
            assert out["ncells"] == len(over) * 5
            _check_distances(out["distances"], Ws, Vs, along, metric, over)
            if len(over) > 1:
                check_summaries(out, out["distances"], Q, (1, 5))
        if len(over) == n_members:
            d, w = posterior_similarity(Ws, Vs, along=along, over=over, pointwise=True)["distances"], whole["distances"]
            assert np.abs(d ** 2 - w ** 2).max() <= 1e-11 * (w ** 2).max()


def test_nearest_of_eight_entries_and_the_library_refuses_nine():
    Ws, Vs = _states(5, 6, 3, 4, 2, seed=31)
    near = (1, 2, 3, 5, 6, 7, 5000, 2 ** 40)                                # 7 > E, and two above every possible group
    out = posterior_similarity(Ws, Vs, nearest=near, pointwise=True)
    assert _no_ties(out["distances"])
    check_summaries(out, out["distances"], (5, 95), near)
    assert (out["p_nearest"][4:] == 1.0).all() and out["nearest"] == near
    lib = _native.load()
    d, ip = _native.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    buf = [np.zeros((6, 6)) for _ in range(5)]
    pn = np.zeros((9, 6, 6))

    def call(nearest):
        nr = np.asarray(nearest, dtype=np.int32)
        return lib.btf_posterior_similarity(0, 5, 6, 3, 4, 2, d(Ws), d(Vs), 0, 0, None, 0, None, 0, ip(nr), len(nr), None, 0, d(buf[0]),
                                            d(buf[1]), None, d(buf[2]), d(buf[3]), d(pn), None, None, 0)
    assert call(range(1, 9)) == _native.BTF_OK
    key = np.where(np.eye(6, dtype=bool), np.nan, out["distances"])
    assert np.array_equal(pn[:8], similarity.neighbours(key, range(1, 9))[2])
    assert call(range(1, 10)) == _native.BTF_EINVAL and b"similarity" in lib.btf_last_error(None)
    assert call((1, 1)) == _native.BTF_EINVAL and call((0,)) == _native.BTF_EINVAL


@pytest.mark.parametrize("along,metric", [("rows", "rms"), ("cols", "cosine")])
def test_tiling_cannot_change_a_bit(along, metric):
    """_scratch_bytes forcing one entity per tile, then tiles of four with an uneven last one: every output is bit-identical
    to the single-tile call."""
    S, E = 6, 11
    N, M = (E, 3) if along == "rows" else (4, E)
    Ws, Vs = _states(S, N, M, 5, 3, seed=41)
    kw = dict(along=along, metric=metric, q=Q, nearest=(1, 2, 4), pairs=[(0, 10), (10, 0), (5, 6), (7, 7)], pointwise=True)
    whole = posterior_similarity(Ws, Vs, **kw)
    per_entity = S * E * 8
    for cap in (1, per_entity, 4 * per_entity + 8):                         # 1 byte: still one entity; then 1; then 4 + 4 + 3
        got = posterior_similarity(Ws, Vs, _scratch_bytes=cap, **kw)
        assert set(got) == set(whole)
        for k, v in whole.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(got[k], v, equal_nan=True), (cap, k)
            else:
                assert got[k] == v, (cap, k)
    _check_distances(whole["distances"], Ws, Vs, along, metric)
