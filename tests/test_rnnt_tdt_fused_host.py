"""The fused token-and-duration training loss without a GPU: the float64 reference of the device tests against torch autograd, the
workspace formula of the header, and the refusals, which are made on the host before anything is enqueued."""
import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_tdt_fused_reference as TF
from nntoolkitcore_amd import capi


def test_float64_reference_matches_autograd():
    c = TF.ragged(5, 6, [0, 1, 2], 2, sigma=0.05)
    for a, b in zip(TF.loss_and_grads(c, "tanh"), TF.torch_fused(c, "tanh", torch.float64)):
        assert np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-11)


def _up(n):
    return (n + 3) & ~3


@pytest.mark.parametrize("B,T,ML,J,V,D", [(3, 7, 5, 67, 254, 5), (1, 3, 300, 4, 3, 3), (16, 200, 40, 640, 1024, 5)])
def test_workspace_is_the_stated_formula(B, T, ML, J, V, D):
    L, cells = capi.load(), B * T * (ML + 1)
    f = lambda g: L.nntk_rnnt_tdt_fused_workspace_floats(B, T, ML, J, V, D, g)
    assert f(0) == L.nntk_rnnt_tdt_workspace_floats(B, T, ML, D, 0)
    assert f(1) == L.nntk_rnnt_tdt_workspace_floats(B, T, ML, D, 1) + _up(cells * J) + _up(J * (V + D)) + _up(32 * (J + 1) * (V + D))
    if V == 1024:
        print("workspace %d floats against %d of the scores alone" % (f(1), cells * (V + D)))
        assert f(1) < cells * (V + D)


GOOD = dict(K.GOOD, dur=[0, 1, 2], sigma=0.0)
BAD = [("durations not ascending", dict(dur=[0, 2, 2]), "durations[2]"), ("no positive duration", dict(dur=[0]), "positive duration"),
       ("nine durations", dict(dur=list(range(9))), "n_durations"),
       ("ring beyond the LDS", dict(ML=568, dur=[0, 16], lab=np.zeros((2, 568), np.int32), ll=[0, 0]), "max_label_len 568"),
       ("T + max_label_len beyond the limit", dict(T=32768 - 2, il=None), "T + max_label_len"), ("J = 0", dict(J=0), "J 0"),
       ("J = 1025", dict(J=1025), "J 1025"), ("V = 8193", dict(V=8193), "V 8193"), ("activation 3", dict(act=3), "activation 3"),
       ("d_dout missing", dict(dout=None), "d_denc, d_dpred, d_dout"), ("only d_denc", dict(dpred=None, dout=None), "d_denc, d_dpred, d_dout"),
       ("misaligned workspace", dict(ws=0x800004), "d_workspace"), ("d_dout overlaps d_out", dict(dout=0x300000), "d_dout overlaps d_out"),
       ("d_denc overlaps the workspace", dict(denc=0x800000 + 32), "d_denc overlaps d_workspace")]


@pytest.mark.parametrize("name,change,word", BAD, ids=K.ids(BAD))
def test_device_form_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them"""
    a, p = dict(GOOD, **change), K.ptr
    rc = capi.load().nntk_rnnt_tdt_fused_loss_device(p(a["enc"]), p(a["pred"]), p(a["out"]), a["B"], a["T"], a["J"], a["V"], K.ints(a["dur"]),
                                                     len(a["dur"]), a["act"], K.ints(a["il"]), K.ints(a["lab"]), K.ints(a["ll"]), a["ML"],
                                                     a["blank"], a["sigma"], p(a["loss"]), p(a["denc"]), p(a["dpred"]), p(a["dout"]), p(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
