"""The token-and-duration transducer loss and its gradient (csrc/hip/rnnt_tdt.hip) against tests/rnnt_tdt_reference.py: the float64
numpy recursion, pinned by tests/test_rnnt_tdt_host.py, which also asserts which rows of these cases have no path.  Tolerance: that of
tests/test_gpu_rnnt.py with its constants -- per row at most FACTOR x the error of the float32 torch restatement on the same case, or
FLOOR where that is smaller; the loss relative to |loss|, the gradient relative to the row's largest |gradient|.

Which case reaches what: ragged V + D = 10, 69, 262 the scalar rows and more than one pass of the wavefront, a row with T_b = 1 < Dmax
and a row without labels; ragged V = 7 (V + D = 12) the 16-byte rows; d12 no zero duration; d12_short and d02 rows without a path on
finite scores (in d02 beside a row with one); d018 a ring deeper than most diagonals are wide; T300 the ring wrapping hundreds of times;
U300 and U512 the general form (U1 > 256), U512 with the dynamic-LDS opt-in; underflow emissions of both heads far below the f32 range."""
import functools
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_tdt_reference as R
from nntoolkitcore_amd import layers as NL

pytestmark = pytest.mark.gpu

TDT_LDS_BYTES, TDT_ENTRY = 160 * 1024, 16            # of nntk_shim.h / rnnt_tdt.hip, mirrored: the ring is (Dmax + 2) U1 entries


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = R.case(name)
    ref = R.tdt_loss_and_grad(c["x"], c["labels"], c["lens"], c["durs"], c["blank"], c["sigma"]) + \
        R.torch_tdt(c["x"], c["labels"], c["lens"], c["durs"], c["blank"], c["sigma"], torch.float32)
    for a in ref:
        a.setflags(write=False)
    return ref


def _run(gpu, c, want_grad=True):
    """NaN in the padding of the scores, and outputs prefilled with NaN: every element has to be written"""
    d = torch.from_numpy(K.with_nan_padding(c)).to(gpu)
    loss = torch.full((d.shape[0],), float("nan"), device=gpu)
    g = torch.full_like(d, float("nan")) if want_grad else None
    NL.rnnt_tdt_loss_device(d, c["labels"], c["durs"], input_lengths=c["lens"], blank=c["blank"], sigma=c["sigma"], want_grad=want_grad,
                            loss=loss, dlogits=g)
    torch.cuda.synchronize()
    return loss.cpu(), (g.cpu() if want_grad else None)


def _check(gpu, name):
    c = R.case(name)
    l64, g64, l32, g32 = _reference(name)
    loss, grad = _run(gpu, c)
    assert not torch.isnan(loss).any() and not torch.isnan(grad).any()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        assert not grad[b, n:].any() and not grad[b, :, len(lab) + 1:].any(), (name, b)      # exact zeros in the padding
        if b in c["inf"]:
            assert l64[b] == math.inf and float(loss[b]) == math.inf and not grad[b].any(), (name, b)
            continue
        assert np.isfinite(l64[b]) and l64[b] > 0
        e, e32 = abs(float(loss[b]) - l64[b]) / l64[b], abs(l32[b] - l64[b]) / l64[b]
        print("%s row %d loss %.9g: err %.2e, torch f32 err %.2e, ratio %.3f" % (name, b, l64[b], e, e32, e / max(e32, 1e-300)))
        gs = np.abs(g64[b]).max()
        ge, ge32 = np.abs(grad[b].double().numpy() - g64[b]).max() / gs, np.abs(g32[b] - g64[b]).max() / gs
        print("%s row %d grad (max |g| %.3g): err %.2e, torch f32 err %.2e, ratio %.3f" % (name, b, gs, ge, ge32, ge / max(ge32, 1e-300)))
        assert e <= max(K.FACTOR * e32, K.FLOOR), (name, b, e, e32)
        assert ge <= max(K.FACTOR * ge32, K.FLOOR), (name, b, ge, ge32)
    return c, loss


@pytest.mark.parametrize("name", R.CASES)
def test_matches_float64(gpu, name):
    c, loss = _check(gpu, name)
    u1, ring = c["x"].shape[2], (max(c["durs"]) + 2) * c["x"].shape[2] * TDT_ENTRY
    assert ring <= TDT_LDS_BYTES
    if name == "U512":                               # the smallest U1 whose ring at Dmax = 4 needs the opt-in
        assert max(c["durs"]) == 4 and ring > K.LDS_OPT_IN >= 6 * (u1 - 1) * TDT_ENTRY and u1 > K.CTC_THREADS
    if name == "underflow":                          # P itself is below the f32 range; its loss is finite all the same
        assert np.exp(-np.float32(_reference(name)[0][0])) == 0.0 and np.isfinite(float(loss[0]))


@pytest.mark.parametrize("name", ["ragged_7_3_0", "d02", "U300"])
def test_loss_only_and_repeats_give_the_same_bits(gpu, name):
    c = R.case(name)
    loss, grad = _run(gpu, c)
    loss2, grad2 = _run(gpu, c)
    loss3, none = _run(gpu, c, want_grad=False)
    assert none is None and torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(loss, loss3)


def test_host_form_equals_the_device_form(gpu):
    c = R.case("ragged_5_4_0")
    loss, grad = _run(gpu, c)
    hl, hg = NL.rnnt_tdt_loss(c["x"], c["labels"], c["durs"], input_lengths=c["lens"], blank=c["blank"])
    assert np.array_equal(hl, loss.numpy()) and np.array_equal(hg, grad.numpy())
