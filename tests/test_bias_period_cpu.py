"""_bias_period: the (inner, outer) row periods handed to the fused
softmax+bias kernel must index the same bias row as torch broadcasting."""

import itertools

import torch

from paddlefleetx_amd.ops.functional import _bias_period


def _broadcast_rows(lead_s, lead_b):
    """bias row read by each logits row under torch broadcasting."""
    nb = 1
    for d in lead_b:
        nb *= d
    return torch.arange(nb).view(*lead_b).expand(*lead_s).reshape(-1)


def _grid():
    K = 5
    for lead_s in itertools.product((1, 2, 3), repeat=3):
        for keep in itertools.product((False, True), repeat=3):
            lead_b = tuple(a if k else 1 for a, k in zip(lead_s, keep))
            yield lead_s + (K,), lead_b + (K,)


def test_bias_period_matches_broadcast():
    n_fused = n_none = 0
    for s_shape, b_shape in _grid():
        lead_s, lead_b = s_shape[:-1], b_shape[:-1]
        bc = [i for i, (a, b) in enumerate(zip(lead_s, lead_b))
              if b == 1 and a != 1]
        run_contiguous = not bc or bc == list(range(bc[0], bc[-1] + 1))
        period = _bias_period(s_shape, b_shape)
        # None exactly when the broadcast dims are not one consecutive run
        assert (period is None) == (not run_contiguous), (s_shape, b_shape)
        if period is None:
            n_none += 1
            continue
        n_fused += 1
        inner, outer = period
        rows = torch.arange(_broadcast_rows(lead_s, lead_s).numel())
        got = (rows // outer) * inner + rows % inner
        want = _broadcast_rows(lead_s, lead_b)
        assert torch.equal(got, want), (s_shape, b_shape, period)
        # the kernel never forms a bias row past the end of the bias
        assert int(got.max()) < _broadcast_rows(lead_b, lead_b).numel()
    assert n_fused > 100 and n_none > 0


def test_bias_period_folding_shapes():
    # pair bias [B, 1, h, Q, K] against logits [B, S, h, Q, K]
    assert _bias_period((2, 3, 2, 5, 37), (2, 1, 2, 5, 37)) == (10, 30)
    assert _bias_period((2, 3, 2, 5, 37), (1, 1, 2, 5, 37)) == (10, 60)
    assert _bias_period((2, 3, 2, 5, 37), (2, 3, 1, 5, 37)) == (5, 10)
    assert _bias_period((2, 3, 2, 5, 37), (2, 3, 2, 5, 37)) == (1, 1)
    # two separate broadcast runs: not expressible, torch fallback
    assert _bias_period((2, 3, 2, 5, 37), (2, 1, 2, 1, 37)) is None


def test_bias_period_refuses_incompatible_shapes():
    assert _bias_period((2, 3, 5), (3, 5)) is None        # rank differs
    assert _bias_period((2, 3, 5), (2, 3, 4)) is None     # last dim differs
    assert _bias_period((2, 3, 5), (2, 2, 5)) is None     # not broadcastable
    assert _bias_period((1, 3, 5), (2, 3, 5)) is None     # bias larger
