"""The pieces of tests/hip_util.py that the GPU tests rest on and that need no
GPU: the split-kernel predicate, the net layout against the library's own
(srcnn_net_offsets is host-only) and the activation sizes."""
import pytest

from hip_util import act_sizes, dims, offsets, ran_x6

NETS = {"default": (64, 32, 9, 1, 5), "example": (32, 16, 9, 1, 5), "wide": (128, 64, 9, 5, 5)}


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


def test_x6_predicate_is_not_vacuous():
    """The names train_fused.hip and train_wide.hip note under either arithmetic."""
    assert ran_x6(["l12x6_fwd", "l3r_d3", "d1x6_d3"])
    assert ran_x6(["wl1x6_fwd", "wgrad2x6"])
    assert not ran_x6(["l12_fwd", "l3r_delta", "d1c_grad12", "slab_reduce"])
    assert not ran_x6(["wide_l1_fwd", "wide_l2_fwd", "d1g16", "wgrad2"])


@pytest.mark.parametrize("name", sorted(NETS))
def test_offsets_are_the_library_s(S, name):
    cfg = NETS[name]
    net = S.Net(*cfg)
    assert offsets(cfg).tolist() == S.net_offsets(net) + [S.net_param_count(net)]


def test_activation_sizes():
    assert dims(NETS["default"], 33, 33) == (25, 25, 25, 25, 21, 21)
    assert dims(NETS["wide"], 33, 33) == (25, 25, 21, 21, 17, 17)
    assert act_sizes(NETS["default"], 33, 33, 7) == (7 * 25 * 25 * 64, 7 * 25 * 25 * 32, 7 * 21 * 21)
    assert act_sizes(NETS["wide"], 35, 31, 3) == (3 * 27 * 23 * 128, 3 * 23 * 19 * 64, 3 * 19 * 15)
