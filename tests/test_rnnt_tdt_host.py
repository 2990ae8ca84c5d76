"""The host side of the token-and-duration transducer calls (csrc/host/rnnt.c): every refusal, made before anything is allocated or
enqueued; and the float64 reference of the device test (tests/rnnt_tdt_reference.py), pinned to enumeration of every path and to float64
autograd, with the rows of the device cases that have no path.  No GPU."""
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_tdt_reference as R
from nntoolkitcore_amd import capi

# (durations, T, U, has a path)
ENUMERATED = [([0, 1, 2], 3, 2, True), ([1, 2], 4, 2, True), ([0, 2], 4, 1, True), ([0, 1, 2, 3, 4], 1, 3, True), ([0, 1, 8], 3, 2, True),
              ([0, 2], 3, 1, False), ([1, 2], 2, 3, False)]


@pytest.mark.parametrize("durs,T,U,finite", ENUMERATED)
@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_reference_equals_enumeration_and_autograd(durs, T, U, finite, sigma):
    rng = np.random.default_rng(T * 10 + U)
    V, blank = 3, 1
    x, lab = rng.uniform(-3, 3, (1, T, U + 1, V + len(durs))), [[0, 2, 0][:U]]
    loss, grad = R.tdt_loss_and_grad(x, lab, [T], durs, blank, sigma)
    walked = R.tdt_row(x[0], lab[0], blank, durs, sigma, enumerate_paths=True)[0]
    assert math.isfinite(loss[0]) == finite and loss[0] == pytest.approx(walked, rel=1e-12)
    tl, tg = R.torch_tdt(x, lab, [T], durs, blank, sigma, torch.float64)
    np.testing.assert_allclose(loss, tl, rtol=1e-12)
    np.testing.assert_allclose(grad, tg, rtol=0, atol=1e-12)
    assert np.abs(grad[..., :V].sum(-1)).max() < 1e-12 and np.abs(grad[..., V:].sum(-1)).max() < 1e-12    # each head's softmax


@pytest.mark.parametrize("name", R.CASES)
def test_device_cases_have_a_path_where_they_say(name):
    c = R.case(name)
    loss, grad = R.tdt_loss_and_grad(c["x"], c["labels"], c["lens"], c["durs"], c["blank"], c["sigma"])
    assert [b for b in range(len(loss)) if loss[b] == math.inf] == c["inf"] and not np.isnan(loss).any()
    assert all(not grad[b].any() for b in c["inf"])


GOOD = dict(K.GOOD, dur=[0, 1, 2], sigma=0.0)
TDT_ONLY = [("no durations", dict(dur=[]), "n_durations"), ("nine durations", dict(dur=list(range(9))), "n_durations"),
            ("durations not ascending", dict(dur=[0, 2, 2]), "ascending"), ("negative duration", dict(dur=[-1, 1]), "negative"),
            ("no positive duration", dict(dur=[0]), "positive"), ("duration above the limit", dict(dur=[0, 17]), "largest duration"),
            ("negative sigma", dict(sigma=-0.1), "sigma"), ("sigma not finite", dict(sigma=math.inf), "sigma"), ("sigma NaN", dict(sigma=math.nan), "sigma"),
            ("ring beyond the LDS", dict(ML=568, dur=[0, 16], lab=np.zeros((2, 568), np.int32), ll=[0, 0]), "max_label_len 568 with the largest duration 16"),
            ("T + max_label_len beyond the halved limit", dict(T=32768 - 2, il=None), "diagonals")]
BAD = K.BAD + K.WS_BAD + K.PLAIN_ONLY + K.LOSS_ONLY + TDT_ONLY


def _call(a):
    p = K.ptr
    return capi.load().nntk_rnnt_tdt_loss_device(p(a["x"]), a["B"], a["T"], a["V"], K.ints(a["dur"]), len(a["dur"]), K.ints(a["il"]),
                                                 K.ints(a["lab"]), K.ints(a["ll"]), a["ML"], a["blank"], a["sigma"], p(a["loss"]), p(a["g"]),
                                                 p(a["ws"]))


@pytest.mark.parametrize("name,change,word", BAD, ids=K.ids(BAD))
def test_device_form_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them"""
    assert _call(dict(GOOD, **change)) == -1 and word in capi.last_error(), (name, capi.last_error())


def test_limits_workspace_and_the_empty_batch():
    L = capi.load()
    f = L.nntk_rnnt_tdt_workspace_floats
    assert f(3, 50, 7, 5, 0) >= (4 + 2 * 5) * 3 * 50 * 8 and f(3, 50, 7, 5, 1) >= f(3, 50, 7, 5, 0) + 8 * 3 * 50 * 8 and f(0, 0, 0, 1, 0) > 0
    assert L.nntk_rnnt_tdt_loss(None, 0, 6, 5, K.ints([1]), 1, None, None, None, 3, 4, 0.0, None, None) == 0 and capi.last_error() == ""
    # the largest lattice inside the limits passes the checks and stops at the first pointer: max_label_len 567 at Dmax = 16
    assert _call(dict(GOOD, ML=567, dur=[0, 16], lab=np.zeros((2, 567), np.int32), ll=[0, 0], x=None)) == -1
    assert "d_logits is NULL" in capi.last_error()
