"""What the GPU tests of the training step share: the fixtures, one function
that runs a step, the ReLU-decision checks and the centred inputs.  A test
module takes the fixtures by name (pytest registers what it finds in the
module's namespace, the autouse one included):

    from step_util import S, _settings  # noqa: F401
"""
import types

import numpy as np
import pytest

import hip_util
from hip_util import D, H, act_sizes, dims, guarded, guards_intact, offsets, ran_x6, segments


@pytest.fixture(scope="module")
def S():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import srcnn_amd
    return srcnn_amd


@pytest.fixture(autouse=True)
def _settings(S):
    """Every test leaves the library on split arithmetic and the auto path,
    whether it passed or raised, and no guarded view registered."""
    yield
    S.set_arith(0)
    S.set_path(0)
    hip_util._GUARDS.clear()


# ----------------------------------------------------------------------------
# one training step
# ----------------------------------------------------------------------------
D1X6_FORMS = ("d1x6_d3", "d1x6_d3_sc")


def ran(path, names, form=None):
    """For run_step(expect=): the step reported `path`, launched every kernel
    of `names` and, with `form`, that one of d1x6's delta3 forms alone."""
    def check(got_path, ks):
        assert got_path == path, got_path
        assert all(k in ks for k in names), (ks, names)
        if form is not None:
            assert [k for k in ks if k in D1X6_FORMS] == [form], ks
    return check


def no_x6(path, ks):
    """For run_step(expect=): no split-arithmetic kernel ran."""
    assert not ran_x6(ks), ks


def run_step(S, cfg, w, h, batch, X, T, params, g0=None, arith=0, guard=False, lazy=None, expect=None,
             hold=False, sq_err=True, ws=None):
    """srcnn_train_fwd_bwd on gradients g0 (default: zeros), or, with lazy =
    (pending gradients, momentum, rates), srcnn_train_fwd_bwd_lazy applying
    that update first.  -> an object with .grads (host), .sq_err, .kernels,
    .path, .params (what the step ran on: the updated ones of a lazy step),
    .ws (the workspace on the device) and .activations() -> host A1, A2, A3
    through srcnn_train_activations.

    guard: an exact-size NaN-filled workspace and every other buffer between
    guard bands of +1e30 (the error cell starts at 0); the bands are checked
    after .grads and .sq_err are read, or, with hold, by .activations() after
    it has read (its outputs' bands too): the caller then owes that call.
    Without guard: plain torch buffers, and the workspace `ws` = (tensor,
    nbytes) if given, else uninitialised with 64 floats of slack.
    expect(path, kernels) runs right after the launch; sq_err=False passes no
    error cell."""
    import torch
    net = S.Net(*cfg)
    S.set_arith(arith)
    views = []

    def buf(a, fill=1e30, inner=None):
        if guard:
            views.append(guarded(a, fill, inner))
            return views[-1]
        return torch.empty(a, dtype=torch.float32, device="cuda") if isinstance(a, (int, np.integer)) else D(a)
    if ws is None:
        nbytes = S.train_workspace_bytes(net, w, h, batch)
        ws = buf(nbytes // 4, float("nan")) if guard else buf(nbytes // 4 + 64)
    else:
        assert not guard
        ws, nbytes = ws
    err = None
    if sq_err:
        err = buf(1, inner=0.0) if guard else torch.zeros(1, dtype=torch.float32, device="cuda")
    Xd, Td, p = buf(X), buf(T), buf(params)
    if lazy is None:
        g = buf(np.zeros(params.size, np.float32) if g0 is None else g0)
        S.train_fwd_bwd(net, Xd, Td, w, h, batch, p, g, err, ws, nbytes)
    else:
        pend, mom, lr = lazy
        g, m, p_out, m_out = buf(pend), buf(mom), buf(params.size), buf(params.size)
        S.train_fwd_bwd_lazy(net, Xd, Td, w, h, batch, p, p_out, m, m_out, g, 0.9, 1e-3, lr, batch, err, ws,
                             nbytes)
    st = types.SimpleNamespace(path=S.last_path(), kernels=S.last_kernels(), ws=ws)
    if expect is not None:
        expect(st.path, st.kernels)
    st.grads = H(g)
    st.sq_err = float(H(err)[0]) if sq_err else None
    st.params = params if lazy is None else H(p_out)

    def activations():
        outs = [buf(n) for n in act_sizes(cfg, w, h, batch)]
        S.train_activations(net, w, h, batch, ws, nbytes, *outs)
        acts = [H(o) for o in outs]
        if guard:
            guards_intact(*views)
            del views[:]
        return acts
    st.activations = activations
    if guard and not hold:
        guards_intact(*views)
        del views[:]
    return st


# ----------------------------------------------------------------------------
# ReLU decisions (tests/test_parity_masks_gpu.py, tests/test_wide_gpu.py)
# ----------------------------------------------------------------------------
# a decision is ambiguous when |exact pre-activation| <= AMBIG x sum |terms|:
# far above fp32's unit roundoff times the term count of any layer here
# (<= 3201 terms x 6e-8 = 2e-4 worst case, ~1e-6 typical), far below the
# activations' own spread
AMBIG = 1e-5


def decisions(cfg, X, w, h, batch, params, A1m):
    """Exact (f64) pre-activations of layers 1 and 2 and the sums of the
    absolute values of their terms; layer 2 is fed the masked exact A1."""
    import srcnn_oracle as orc
    n1, n2, f1, f2, f3 = cfg
    W1, B1, W2, B2, W3, B3 = segments(cfg, np.asarray(params, np.float64))
    w1, h1, w2, h2, _, _ = dims(cfg, w, h)
    F = orc.f64
    pre1 = F.conv_fwd(X, W1, B1, w, h, 1, n1, f1, 0, batch)
    mag1 = F.conv_fwd(np.abs(X), np.abs(W1), np.abs(B1), w, h, 1, n1, f1, 0, batch)
    pre2 = F.conv_fwd(A1m, W2, B2, w1, h1, n1, n2, f2, 0, batch)
    mag2 = F.conv_fwd(np.abs(A1m), np.abs(W2), np.abs(B2), w1, h1, n1, n2, f2, 0, batch)
    return pre1, mag1, pre2, mag2


def check_flips(what, mask, pre, mag):
    """Every HIP decision that differs from the exact one is a rounding case."""
    exact = pre > 0
    flips = mask != exact
    amb = np.abs(pre) <= AMBIG * mag
    n_flip, n_amb = int(flips.sum()), int(amb.sum())
    bad = int((flips & ~amb).sum())
    assert bad == 0, "%s: %d ReLU decisions differ from the exact sign outside the rounding band" % (what, bad)
    return n_flip, n_amb


# ----------------------------------------------------------------------------
# inputs whose ReLU' masks are mixed
# ----------------------------------------------------------------------------
def mid(a):
    """Midway between the two middle values (at the median itself one value
    would be 0 up to rounding and its ReLU decision a coin toss between any
    two fp32 summation orders)."""
    s = np.sort(np.asarray(a, np.float64), axis=0)
    k = s.shape[0] // 2
    return 0.5 * (s[k - 1] + s[k])


def centre_params(cfg, X, w, h, batch, params, dead=(), all_positive=False):
    """In place: layer 2's biases to minus mid() of each channel's
    pre-activation, so that every channel's ReLU' mask is mixed (as drawn with
    sd 0.05, B2 decides a channel's sign almost everywhere: about half of the
    channels are dead and the rest always on); the channels `dead` then to
    -1e3; then layer 3's bias so that half of A3 is positive (delta3 is masked
    by A3 > 0), or (all_positive) every A3 by at least 0.1."""
    import srcnn_oracle as orc
    n1, n2, f1, f2, f3 = cfg
    off = offsets(cfg)
    w1, h1 = dims(cfg, w, h)[:2]
    A1 = orc.conv_fwd(X, params[off[0]:off[1]], params[off[1]:off[2]], w, h, 1, n1, f1, 1, batch)
    Z = orc.conv_fwd(A1, params[off[2]:off[3]], np.zeros(n2, np.float32), w1, h1, n1, n2, f2, 0, batch)
    params[off[3]:off[4]] = (-mid(np.asarray(Z).reshape(-1, n2))).astype(np.float32)
    if dead:
        params[off[3] + np.array(dead)] = -1e3
    a3 = np.asarray(orc.forward(cfg, X, w, h, batch, params), np.float64).ravel()
    params[-1] -= np.float32(a3.min() - 0.1 if all_positive else mid(a3))
