"""BTF_OPT_GRAM_ASIDE: the columns' shares V_j'V_j of the Gram as a side task of the NEXT W accumulation launch.

With the option on (the default) the tails of the fused V launch store V and leave; the shares the next `_resample_W`
(factor.py:349-362: Q = X'CX + I / sigma2) needs are formed beside the stream of its accumulation launch, from V as
stored, by the tails' own device function (gram_share_part / gram_share_total) - or by a small launch of that function
where the side task does not apply.  These are the same operations in the same order on the same doubles, so every
chain here must agree BIT FOR BIT with option 0 (the tails form the shares), and no launch is added to the step.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _synth(N, M, T, R, K, seed=3):
    rs = np.random.RandomState(seed)
    Wt = rs.normal(size=(N, K))
    Vt = 0.1 * np.cumsum(rs.normal(size=(M, T, K)), axis=1)
    return np.einsum("nk,mtk->nmt", Wt, Vt)[..., None] + rs.normal(0, 0.5, size=(N, M, T, R))


def _make(dims, aside, rng="device", fused=1, seed=11, sampler="spectral"):
    from functionalmf_amd import _native
    from functionalmf_amd.factor import GaussianBayesianTensorFiltering
    N, M, T, R, K = dims
    np.random.seed(seed)
    m = GaussianBayesianTensorFiltering(N, M, T, nembeds=K, tf_order=2, sigma2_init=0.5, lam2_init=0.1, nu2_init=1.0,
                                        rng=rng, device_seed=5, compat="reference", sampler=sampler)
    m._ctx.call("btf_set_option", _native.OPT_FUSED_STEP, int(fused))
    m._ctx.call("btf_set_option", _native.OPT_GRAM_ASIDE, int(aside))
    return m


def _launches(m):
    return {k: v[1] for k, v in m._ctx.kernel_times().items() if v[1]}


def _chain(m, Y, steps=3, sweeps=2):
    """3 W+V steps, then 2 full sweeps; the state after each leg."""
    np.random.seed(21)
    m._bind_data(Y)
    m._ctx.kernel_times()
    for _ in range(steps):
        m._resample_W(Y)
        m._resample_V(Y)
    m.sync()                                               # (raises if a hand-off timed out or a factor failed)
    la = _launches(m)
    out = [m.W.copy(), m.V.copy()]
    for _ in range(sweeps):
        m.resample(Y)
    m.sync()
    out += [m.W.copy(), m.V.copy()]
    return out, la


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        assert np.array_equal(x, y)


# (N, M, T, R, K).  ndepth 32 / 64 / 128: four, two, one column per 128-output tile; ncols 1, 3, 5: a dead column group in the
# last tile; nrows 24 and 70: a first w_solve workgroup with the triangular rows, ordinary ones behind it, a ragged last
# one; nembeds 1, 5, 6: the dataflow tail (ng = 16, 16, 12 groups per share), 7 and 8: the barrier tail (ng = 9, 7).
# The last two have more columns than one w_solve workgroup sums in a batch (8 lanes' worth: 136 at nembeds 5, 56 at nembeds
# 8): there the sum side workgroup of the W launch runs too, and waits for the share workgroups in front of it.
SHAPES = [(24, 3, 64, 2, 5), (70, 5, 32, 2, 5), (70, 1, 128, 1, 5), (24, 5, 64, 2, 1), (70, 3, 32, 2, 6), (24, 1, 32, 2, 6),
          (24, 3, 128, 2, 7), (70, 5, 64, 2, 8), (24, 140, 32, 1, 5), (70, 60, 32, 1, 8)]


@pytest.mark.parametrize("dims", SHAPES)
def test_aside_walks_the_same_chain_bit_for_bit(dims, monkeypatch):
    # two columns per share workgroup: ncols 3 and 5 give several share workgroups with a ragged last one
    monkeypatch.setenv("BTF_SHARE_CPW", "2")
    Y = _synth(*dims)
    (a, la), (b, lb) = _chain(_make(dims, 1), Y), _chain(_make(dims, 0), Y)
    _same(a, b)
    # three launches per step either way: no launch was added, none for the shares
    la.pop("prior_band", None), lb.pop("prior_band", None)
    assert la == {"w_accum": 3, "w_solve": 3, "v_accum": 3}, la
    assert lb == {"w_accum": 3, "w_solve": 3, "v_accum": 3}, lb


def test_aside_default_columns_per_share_workgroup():
    dims = (70, 21, 64, 2, 5)                              # the default, at most eight columns per share workgroup: 7, 7, 7
    Y = _synth(*dims)
    (a, _), (b, _) = _chain(_make(dims, 1), Y), _chain(_make(dims, 0), Y)
    _same(a, b)


def test_aside_host_normals():
    dims = (70, 5, 64, 2, 5)
    Y = _synth(*dims)
    (a, _), (b, _) = _chain(_make(dims, 1, rng="host"), Y), _chain(_make(dims, 0, rng="host"), Y)
    _same(a, b)


def test_aside_four_launch_form_walks_the_same_chain():
    """BTF_OPT_FUSED_STEP 0 (four launches): the sampler launch of its own emits the shares itself, whatever the option says.
    It walks the chain of the three-launch step bit for bit where the two forms are bit-identical at all - the barrier
    tail (BTF_OPT_FUSED_DATAFLOW 0), whose shares now come from the W launch's side task.  The library's default, the
    dataflow tail, groups the column sums over fewer waves: equal to the four-launch form to rounding, with the bound
    tests/test_gpu_fused.py pins for three steps (1e-11 of the factors' scale), as before this option existed."""
    from functionalmf_amd import _native
    dims = (70, 5, 64, 2, 5)
    Y = _synth(*dims)
    (a, la), (a0, _) = _chain(_make(dims, 1, fused=0), Y, sweeps=0), _chain(_make(dims, 0, fused=0), Y, sweeps=0)
    la.pop("prior_band", None)
    assert la == {"w_accum": 3, "w_solve": 3, "v_accum": 3, "v_banded": 3}, la
    _same(a, a0)
    m = _make(dims, 1)
    m._ctx.call("btf_set_option", _native.OPT_FUSED_DATAFLOW, 0)
    b, lb = _chain(m, Y, sweeps=0)
    lb.pop("prior_band", None)
    assert lb == {"w_accum": 3, "w_solve": 3, "v_accum": 3}, lb
    _same(a, b)
    c, _ = _chain(_make(dims, 1), Y, sweeps=0)             # the default: the dataflow tail
    for x, y in zip(a, c):
        assert np.abs(x - y).max() < 1e-11 * np.abs(x).max()


def test_shares_owed_are_those_of_the_last_V():
    dims = (24, 5, 64, 2, 5)
    Y = _synth(*dims)
    outs = []
    for aside in (1, 0):
        m = _make(dims, aside)
        np.random.seed(21)
        m._bind_data(Y)
        m._resample_W(Y)
        m._resample_V(Y)
        m._resample_V(Y)
        m._resample_W(Y)
        m._resample_V(Y)
        m.sync()
        outs.append([m.W.copy(), m.V.copy()])
    _same(*outs)


@pytest.mark.parametrize("how", ["option", "fused_w", "nu2"])
def test_shares_are_paid_on_demand(how):
    """Between V and W: the option is switched off (btf_set_option pays what is owed), the next W half-sweep runs the solve
    as the tail of its accumulation launch (BTF_OPT_FUSED_STEP 2: its owners read the shares inside the launch, so a launch
    of their own forms them first), or nu2 | rest is drawn (which leaves the debt alone)."""
    from functionalmf_amd import _native
    dims = (70, 5, 64, 2, 5)
    Y = _synth(*dims)
    outs = []
    for aside in (1, 0):
        m = _make(dims, aside)
        np.random.seed(21)
        m._bind_data(Y)
        m._resample_W(Y)
        m._resample_V(Y)
        m._ctx.kernel_times()
        if how == "option":
            m._ctx.call("btf_set_option", _native.OPT_GRAM_ASIDE, 0)
        elif how == "fused_w":
            m._ctx.call("btf_set_option", _native.OPT_FUSED_STEP, 2)
        else:
            np.random.seed(5)
            m._resample_nu2(Y)
        m._resample_W(Y)
        m._resample_V(Y)
        m.sync()
        la = _launches(m)
        if how != "nu2":
            assert la.get("gram", 0) == (1 if aside else 0), la
        outs.append([m.W.copy(), m.V.copy()])
    _same(*outs)


@pytest.mark.parametrize("variant", ["heldout", "weighted"])
def test_incomplete_data_is_untouched(variant):
    """Held-out curves (curve counts) and single missing replicates (weighted data) never run the fused V launch: neither
    run here reaches the code the option switches, so this only shows that option 1 does nothing on those paths."""
    dims = (24, 5, 64, 3, 5)
    Y = _synth(*dims)
    if variant == "heldout":
        Y[:2, :2] = np.nan
    else:
        Y[np.random.RandomState(4).rand(*Y.shape[:3]) < 0.05, 0] = np.nan
    outs = []
    for aside in (1, 0):
        m = _make(dims, aside, sampler="auto")
        np.random.seed(21)
        m._bind_data(Y)
        for _ in range(3):
            m._resample_W(Y)
            m._resample_V(Y)
        m.sync()
        outs.append([m.W.copy(), m.V.copy()])
    _same(*outs)
