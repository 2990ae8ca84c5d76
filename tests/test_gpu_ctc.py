"""CTC loss, its gradient with respect to the probabilities, and greedy decoding (csrc/hip/ctc.hip) against torch on the CPU.

Reference: ``torch.nn.functional.ctc_loss`` in float64, ``reduction='none'``, fed ``log(probs)`` with ``probs`` -- the float32 values the
library receives -- as a float64 leaf.  One correction is applied to what autograd returns: torch's CTC backward is written for
log-probabilities that come out of a log_softmax and returns ``exp(lp) - occupancy`` instead of ``-occupancy`` (the extra term cancels
inside log_softmax's own backward).  Through ``log`` that is ``1 - occupancy / p`` for every class of every frame t < input_length, so
the true derivative -- what the library documents and what a softmax layer's gradient call consumes (the end-to-end test below pins
that) -- is autograd's result minus 1 on those frames.  The same correction is applied to the float32 torch result that sets the tolerance.

Tolerance (per row; the gradient relative to the row's largest |gradient|): the library's error against float64 is at most FACTOR x
the error of torch's own float32 ctc_loss against float64 on the same inputs, or 16 * 2^-24 where that is larger."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
FACTOR = 2.0          # the issue allows 4; measured: at most 1.0 (loss; the float32 rounding of the result itself) and 0.35 (gradient)
# measured on MI355X at the large shapes (states_801 / _1027 / _2481, wide_C3000 / C3001 / C9001 / C12301, max_label_len 4000): loss at most
# 1.0 as before; gradient at most 0.34 (max_label_len 4000), 0.075 among the wide cases and 0.002 among the long transcripts, where torch's
# float32 log-space gradient is off by 5e-4 .. 4e-3 of the row's largest entry and the library by 3e-7 .. 1.8e-6


def _softmax(rng, B, T, Cc):
    z = torch.from_numpy(rng.uniform(-2, 2, (B, T, Cc)).astype(np.float32))
    return torch.softmax(z, -1).numpy()


def _no_repeat(rng, L, Cc, blank):
    """L random labels, none equal to its neighbour: feasible in L frames"""
    classes = [k for k in range(Cc) if k != blank]
    out = []
    for _ in range(L):
        k = classes[int(rng.integers(len(classes)))]
        while out and k == out[-1]:
            k = classes[int(rng.integers(len(classes)))]
        out.append(k)
    return out


def _case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "edges_T1":
        return dict(probs=_softmax(rng, 2, 1, 5), labels=[[], [3]], lens=[1, 1], blank=0)
    if name == "edges_T12":
        labels = [[], [0], [0, 1, 2], [0, 1, 0, 2, 3, 1], [1, 1], [1, 1], [2], [], [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]]
        return dict(probs=_softmax(rng, len(labels), 12, 5), labels=labels, lens=[12, 10, 12, 11, 3, 2, 0, 0, 12], blank=4)
    if name == "states_63_65_67":
        return dict(probs=_softmax(rng, 3, 70, 29), labels=[[(i % 28) + 1 for i in range(L)] for L in (31, 32, 33)], lens=[70, 69, 70], blank=0)
    if name == "states_261":
        return dict(probs=_softmax(rng, 1, 270, 29), labels=[[(i % 28) + 1 for i in range(130)]], lens=[270], blank=0)
    if name == "one_class_repeated":
        return dict(probs=_softmax(rng, 1, 45, 29), labels=[[7] * 20], lens=[45], blank=0)
    if name == "range_T400":
        return dict(probs=_softmax(rng, 2, 400, 30), labels=[_no_repeat(rng, 60, 30, 0), _no_repeat(rng, 130, 30, 0)], lens=[400, 390], blank=0)
    if name == "wide_C1000":
        return dict(probs=_softmax(rng, 2, 60, 1000), labels=[_no_repeat(rng, 20, 1000, 0), _no_repeat(rng, 5, 1000, 0)], lens=[60, 57], blank=0)
    if name == "odd_C37":
        return dict(probs=_softmax(rng, 2, 60, 37), labels=[_no_repeat(rng, 20, 37, 36), [5, 5, 9, 5, 5]], lens=[60, 33], blank=36)
    if name in STATES:                                # long transcripts: labels without adjacent repeats, blank 0
        (B, T, Cc), lls, ils = STATES[name]
        return dict(probs=_softmax(rng, B, T, Cc), labels=[[(i % (Cc - 1)) + 1 for i in range(L)] for L in lls], lens=list(ils), blank=0)
    if name in WIDE:                                  # large vocabularies: blank C - 1, a repeated class, row 1 shorter than T; C is odd,
        B, T, Cc = WIDE[name]                         # so most gradient rows start off a 16-byte boundary
        return dict(probs=_softmax(rng, B, T, Cc), labels=[[7, 7, Cc - 2], [Cc - 3, 2, 2]], lens=[T, T - 1], blank=Cc - 1)
    raise KeyError(name)


# name: ((B, T, C), label lengths, input lengths)
STATES = {"states_801": ((2, 900, 30), (400, 257), (900, 880)),
          "states_1027": ((1, 600, 30), (513,), (600,)),
          "states_2481": ((2, 1300, 30), (1240, 3), (1300, 1290))}
# (wide_C3001: wide_C3000 with rows that start off a 16-byte boundary, so that the gradient's head and tail stores run with nt < TT too)
WIDE = {"wide_C3000": (2, 7, 3000), "wide_C3001": (2, 7, 3001), "wide_C9001": (2, 5, 9001), "wide_C12301": (2, 6, 12301)}
CASES = ("edges_T1", "edges_T12", "states_63_65_67", "states_261", "one_class_repeated", "range_T400", "wide_C1000", "odd_C37",
         "states_801", "states_1027", "states_2481", "wide_C3000", "wide_C3001", "wide_C9001", "wide_C12301")


# ---- which code path of ctc.hip a shape takes: its constants, mirrored, so that a moved threshold turns the premise assertions red ----

CTC_THREADS = 256                    # ctc.hip:24
CTC_GRAD_LDS_FLOATS = 8192           # ctc.hip:25
CTC_GRAD_MAX_C = 32768               # ctc.hip:26
CTC_LDS_LIMIT = 160 * 1024           # ctc.hip:27
LDS_OPT_IN = 48 * 1024               # ctc.hip:315 and :329: a larger request goes through nntk_set_max_dynamic_lds first
ARGMAX_MAX_GRID, ARGMAX_FRAMES = 16384, 4            # ctc.hip:344 (the grid's cap) and :236 (a wavefront per frame, four per workgroup)


def _alpha_beta_path(max_label_len):
    """(Smax, NJ of the ctc_alpha_beta_kernel instantiation, its LDS request in bytes)"""
    smax = 2 * max_label_len + 1                                                             # ctc.hip:298
    lds = ((smax * 4 + 15) & ~15) + 2 * (smax + 4) * 8                                       # ctc.hip:299
    nj = 1 if smax <= CTC_THREADS else 2 if smax <= 2 * CTC_THREADS else 4 if smax <= 4 * CTC_THREADS else 0     # ctc.hip:319-322
    return smax, nj, lds


def _grad_path(Cc):
    """(TT = timesteps staged per workgroup of ctc_grad_kernel, its LDS request in bytes)"""
    tt = min(max(CTC_GRAD_LDS_FLOATS // Cc, 1), 16)                                          # ctc.hip:326-327
    return tt, tt * Cc * 4                                                                   # ctc.hip:328


# what each large-shape case is there to reach: (NJ, alpha/beta LDS opt-in, TT, frames in the last time block, gradient LDS opt-in)
PREMISES = {"states_801": (4, False, 16, 4, False), "states_1027": (0, False, 16, 8, False), "states_2481": (0, True, 16, 4, False),
            "wide_C3000": (1, False, 2, 1, False), "wide_C3001": (1, False, 2, 1, False),
            "wide_C9001": (1, False, 1, 1, False), "wide_C12301": (1, False, 1, 1, True)}


def _assert_premise(name, c):
    B, T, Cc = c["probs"].shape
    lls = [len(r) for r in c["labels"]]
    smax, nj, lds = _alpha_beta_path(max(lls))
    tt, glds = _grad_path(Cc)
    assert (nj, lds > LDS_OPT_IN, tt, T - (T - 1) // tt * tt, glds > LDS_OPT_IN) == PREMISES[name], (name, smax, nj, lds, tt, glds)
    assert lds <= CTC_LDS_LIMIT and Cc <= CTC_GRAD_MAX_C
    for b in range(B):
        assert all(x != y for x, y in zip(c["labels"][b], c["labels"][b][1:])) or name in WIDE
    if name == "states_801":
        assert smax == 801 and all(2 * L + 1 > 2 * CTC_THREADS for L in lls)                 # both rows have states in the third and fourth slot
    if name == "states_1027":
        assert smax == 1027 > 4 * CTC_THREADS
    if name == "states_2481":
        assert smax == 2481 and lds == 49696 and 2 * lls[1] + 1 <= CTC_THREADS               # a short row inside a large-Smax batch
    if name in WIDE:
        assert (Cc % 4 != 0) == (name != "wide_C3000") and c["blank"] == Cc - 1 and c["lens"][1] < T
        assert any(x == y for r in c["labels"] for x, y in zip(r, r[1:])) and len(set(c["labels"][0])) < len(c["labels"][0])
    if name == "wide_C12301":
        assert glds == 49204


def _torch_ctc(probs, labels, lens, blank, dtype):
    """loss rows and the true d loss / d probs from torch on the CPU (see the module docstring); an impossible row: +inf, zeros"""
    B, T, Cc = probs.shape
    p = torch.from_numpy(probs).to(dtype).requires_grad_(True)
    ll = torch.tensor([len(r) for r in labels], dtype=torch.long)
    tgt = torch.zeros((B, max(1, int(ll.max()))), dtype=torch.long)
    for b, r in enumerate(labels):
        tgt[b, :len(r)] = torch.tensor(r, dtype=torch.long)
    il = torch.tensor(lens, dtype=torch.long)
    loss = torch.nn.functional.ctc_loss(torch.log(p).transpose(0, 1), tgt, il, ll, blank=blank, reduction="none")
    ok = torch.isfinite(loss)
    g = torch.zeros_like(p)
    if ok.any():
        g = torch.autograd.grad(loss[ok].sum(), p)[0].detach().clone()
        live = (torch.arange(T)[None, :] < il[:, None]) & ok[:, None]
        g[live] -= 1.0
        g[~ok] = 0.0
    return loss.detach().double().numpy(), g.double().numpy()


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = _case(name)
    clean = np.where(np.isnan(c["probs"]), np.float32(1.0 / c["probs"].shape[2]), c["probs"])
    l64, g64 = _torch_ctc(clean, c["labels"], c["lens"], c["blank"], torch.float64)
    l32, g32 = _torch_ctc(clean, c["labels"], c["lens"], c["blank"], torch.float32)
    for a in (l64, g64, l32, g32):
        a.setflags(write=False)
    return l64, g64, l32, g32


def _with_nan_tail(c):
    p = c["probs"].copy()
    for b, n in enumerate(c["lens"]):
        p[b, n:] = np.nan
    return p


def _run(gpu, probs, labels, lens, blank, want_grad=True):
    x = torch.from_numpy(probs).to(gpu)
    loss = torch.full((probs.shape[0],), float("nan"), device=gpu)
    g = torch.full_like(x, float("nan")) if want_grad else None
    NL.ctc_loss_device(x, labels, input_lengths=lens, blank=blank, want_grad=want_grad, loss=loss, dprobs=g)
    torch.cuda.synchronize()
    return loss.cpu(), (g.cpu() if want_grad else None)


def _assert_close(tag, loss, grad, l64, g64, l32, g32, skip=None):
    """skip: boolean mask of gradient entries left out of the comparison"""
    loss, grad = loss.double().numpy(), grad.double().numpy()
    for b in range(loss.shape[0]):
        if not np.isfinite(l64[b]):
            assert loss[b] == np.inf and not grad[b].any(), (tag, b, loss[b])
            continue
        sc = abs(l64[b])
        if sc == 0.0:
            assert loss[b] == 0.0, (tag, b, loss[b])
        else:
            e, e32 = abs(loss[b] - l64[b]) / sc, abs(l32[b] - l64[b]) / sc
            print("%s row %d loss %.9g: err %.2e, torch f32 err %.2e, ratio %.3f" % (tag, b, l64[b], e, e32, e / max(e32, 1e-300)))
            assert e <= max(FACTOR * e32, FLOOR), (tag, b, e, e32)
        keep = np.ones(g64[b].shape, bool) if skip is None else ~skip[b]
        gs = np.abs(g64[b][keep]).max() if keep.any() else 0.0
        if gs == 0.0:
            assert not grad[b][keep].any(), (tag, b)
            continue
        e = np.abs(grad[b] - g64[b])[keep].max() / gs
        e32 = np.abs(g32[b] - g64[b])[keep].max() / gs
        print("%s row %d grad (max |g| %.3g): err %.2e, torch f32 err %.2e, ratio %.3f" % (tag, b, gs, e, e32, e / max(e32, 1e-300)))
        assert e <= max(FACTOR * e32, FLOOR), (tag, b, e, e32)


@pytest.mark.parametrize("name", CASES)
def test_loss_and_gradient_match_torch_float64(gpu, name):
    """cases 1-4 of the issue: edges (NaN behind every row's length), S around one wavefront and beyond the workgroup, one class
    repeated, T = 400 range, C = 1000 and C = 37 with the output prefilled with NaN; the large shapes (PREMISES): four states per lane
    (NJ = 4), the any-S kernel (NJ = 0) without and with the dynamic-LDS opt-in, one and two gradient rows staged per workgroup"""
    c = _case(name)
    if name in PREMISES:
        _assert_premise(name, c)
    loss, grad = _run(gpu, _with_nan_tail(c), c["labels"], c["lens"], c["blank"])
    assert not torch.isnan(grad).any() and not torch.isnan(loss).any()
    for b, n in enumerate(c["lens"]):
        assert not grad[b, n:].any(), (name, b)                       # exact zeros behind the row's length
    l64, g64, l32, g32 = _reference(name)
    if name == "edges_T12":
        assert l64[5] == np.inf and l64[6] == np.inf and l64[7] == 0.0 and np.isfinite(l64[[0, 1, 2, 3, 4, 8]]).all()
    if name == "range_T400":
        assert (l64 > 900).all() and (l64 < 1300).all()
    _assert_close(name, loss, grad, l64, g64, l32, g32)


def test_zeros_in_the_probabilities(gpu):
    """case 5: exact zeros on and off the label path, and one row whose every path is killed"""
    rng = np.random.default_rng(55)
    B, T, Cc, blank = 3, 14, 6, 0
    labels = [[1, 2, 2, 3], [4, 1], [2, 5]]
    lens = [14, 12, 14]
    p = _softmax(rng, B, T, Cc)
    p[0, 3, 2] = 0; p[0, 7, 0] = 0; p[0, 5, 5] = 0; p[0, 0, 3] = 0; p[0, 13, 0] = 0       # on the path (2, blank) and off it (5; 3 at t = 0)
    p[1, 2, 4] = 0; p[1, 2, 3] = 0; p[1, 11, 1] = 0
    p[2, 6, :] = 0; p[2, 6, 1] = 1.0                                                         # frame 6 admits only class 1: not in the label
    loss, grad = _run(gpu, p, labels, lens, blank)
    assert not torch.isnan(grad).any()
    assert not grad[torch.from_numpy(p == 0)].any()
    assert loss[2] == np.inf and not grad[2].any()
    # the reference takes 1e-300 (float32: 1e-30) for 0: the same loss and, away from those entries, the same gradient
    l64, g64 = _torch_ctc(np.where(p == 0, 1e-300, p.astype(np.float64))[:2], labels[:2], lens[:2], blank, torch.float64)
    l32, g32 = _torch_ctc(np.where(p == 0, np.float32(1e-30), p)[:2], labels[:2], lens[:2], blank, torch.float32)
    l0, _ = _torch_ctc(p[:2].copy(), labels[:2], lens[:2], blank, torch.float64)            # ... and the loss with the zeros themselves
    np.testing.assert_allclose(l0, l64, rtol=1e-12)
    _assert_close("zeros", loss[:2], grad[:2], l64, g64, l32, g32, skip=(p[:2] == 0))


def test_determinism_and_row_independence(gpu):
    """case 6 on the T = 400 inputs: repeated call, row 0 alone, and the loss without a gradient -- identical bits"""
    c = _case("range_T400")
    p = _with_nan_tail(c)
    loss, grad = _run(gpu, p, c["labels"], c["lens"], c["blank"])
    loss2, grad2 = _run(gpu, p, c["labels"], c["lens"], c["blank"])
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    loss1, grad1 = _run(gpu, p[:1], c["labels"][:1], c["lens"][:1], c["blank"])
    assert torch.equal(loss1, loss[:1]) and torch.equal(grad1, grad[:1])
    loss3, none = _run(gpu, p, c["labels"], c["lens"], c["blank"], want_grad=False)
    assert none is None and torch.equal(loss3, loss)


def test_argument_errors_write_nothing(gpu):
    """case 7: -1, a message, and the outputs as they were"""
    L = capi.load()
    B, T, Cc, ML = 2, 6, 5, 3
    x = torch.full((B, T, Cc), 0.2, device=gpu)
    ws = torch.empty(L.nntk_ctc_workspace_floats(B, T, ML), device=gpu)
    dp = lambda t: C.c_void_p(t.data_ptr())
    good = dict(il=[6, 4], lab=[[1, 2, 0], [3, 0, 0]], ll=[2, 1], blank=4)
    bad = [dict(il=[7, 4]), dict(il=[6, -1]), dict(ll=[4, 1]), dict(ll=[2, -1]), dict(lab=[[1, 4, 0], [3, 0, 0]]),
           dict(lab=[[1, 5, 0], [3, 0, 0]]), dict(lab=[[-1, 2, 0], [3, 0, 0]]), dict(blank=5), dict(blank=-1)]
    for change in bad:
        a = dict(good, **change)
        loss, g = torch.full((B,), 7.0, device=gpu), torch.full((B, T, Cc), 7.0, device=gpu)
        il, lab, ll = np.asarray(a["il"], np.int32), np.asarray(a["lab"], np.int32), np.asarray(a["ll"], np.int32)
        rc = L.nntk_ctc_loss_device(dp(x), B, T, Cc, il.ctypes.data_as(capi.ip), lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip),
                                    ML, a["blank"], dp(loss), dp(g), dp(ws))
        assert rc == -1 and capi.last_error() != "", change
        torch.cuda.synchronize()
        assert (loss == 7.0).all() and (g == 7.0).all(), change
    for change in (dict(il=[7, 4]), dict(il=[-2, 4]), dict(blank=5), dict(blank=-1)):
        a = dict(good, **change)
        out, n = torch.full((B, T), 7, dtype=torch.int32, device=gpu), torch.full((B,), 7, dtype=torch.int32, device=gpu)
        il = np.asarray(a["il"], np.int32)
        rc = L.nntk_ctc_greedy_decode_device(dp(x), B, T, Cc, il.ctypes.data_as(capi.ip), a["blank"], dp(out), dp(n))
        assert rc == -1 and capi.last_error() != "", change
        torch.cuda.synchronize()
        assert (out == 7).all() and (n == 7).all(), change


def _capi_loss(x, il, lab, ll, blank, loss, g):
    """nntk_ctc_loss_device through the C boundary with a padded label array [B][max_label_len]: (return code, message)"""
    L = capi.load()
    B, T, Cc = x.shape
    il, lab, ll = np.asarray(il, np.int32), np.ascontiguousarray(lab, np.int32), np.asarray(ll, np.int32)
    ws = torch.empty(L.nntk_ctc_workspace_floats(B, T, lab.shape[1]), device=x.device)
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = L.nntk_ctc_loss_device(dp(x), B, T, Cc, il.ctypes.data_as(capi.ip), lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip),
                                lab.shape[1], blank, dp(loss), dp(g), dp(ws))
    torch.cuda.synchronize()
    return rc, capi.last_error()


def test_documented_label_limit_and_its_refusal(gpu):
    """max_label_len = 4000, the limit the shim's message names, runs (the any-S kernel at 160 KB of LDS) and matches float64;
    4200 is refused with a message before anything is written"""
    rng = np.random.default_rng(4000)
    B, T, Cc, blank = 2, 3, 5, 0
    p = _softmax(rng, B, T, Cc)
    lens, ll = [3, 2], [1, 0]
    p[1, 2:] = np.nan
    x = torch.from_numpy(p).to(gpu)
    for ML, fits in ((4000, True), (4200, False)):
        smax, nj, lds = _alpha_beta_path(ML)
        assert nj == 0 and lds > LDS_OPT_IN and (lds <= CTC_LDS_LIMIT) == fits, (ML, smax, nj, lds)      # 160,096 and 168,096 bytes
        lab = np.zeros((B, ML), np.int32)
        lab[0, 0] = 3
        loss, g = torch.full((B,), 7.0, device=gpu), torch.full((B, T, Cc), 7.0, device=gpu)
        rc, msg = _capi_loss(x, lens, lab, ll, blank, loss, g)
        if not fits:
            assert rc == -1 and "max_label_len" in msg, (rc, msg)
            assert (loss == 7.0).all() and (g == 7.0).all()
            continue
        assert rc == 0, msg
        loss, g = loss.cpu(), g.cpu()
        assert not torch.isnan(g).any() and not g[1, 2:].any()
        clean = np.where(np.isnan(p), np.float32(1.0 / Cc), p)
        l64, g64 = _torch_ctc(clean, [[3], []], lens, blank, torch.float64)
        l32, g32 = _torch_ctc(clean, [[3], []], lens, blank, torch.float32)
        _assert_close("max_label_len_4000", loss, g, l64, g64, l32, g32)


def test_gradient_class_limit(gpu):
    """C = 32769: one class more than a gradient row staged in the LDS holds.  The call with a gradient is refused and writes nothing;
    the loss alone has no such limit and matches float64"""
    rng = np.random.default_rng(32769)
    B, T, Cc, blank = 1, 3, 32769, 0
    assert Cc == CTC_GRAD_MAX_C + 1
    p = _softmax(rng, B, T, Cc)
    labels = [[Cc - 1, 5]]
    x = torch.from_numpy(p).to(gpu)
    loss, g = torch.full((B,), 7.0, device=gpu), torch.full((B, T, Cc), 7.0, device=gpu)
    rc, msg = _capi_loss(x, [T], np.asarray(labels, np.int32), [2], blank, loss, g)
    assert rc == -1 and "32768" in msg, (rc, msg)
    assert (loss == 7.0).all() and (g == 7.0).all()
    rc, msg = _capi_loss(x, [T], np.asarray(labels, np.int32), [2], blank, loss, None)
    assert rc == 0, msg
    l64, _ = _torch_ctc(p, labels, [T], blank, torch.float64)
    l32, _ = _torch_ctc(p, labels, [T], blank, torch.float32)
    e, e32 = abs(float(loss[0]) - l64[0]) / l64[0], abs(l32[0] - l64[0]) / l64[0]
    print("C = 32769 loss %.9g: err %.2e, torch f32 err %.2e" % (l64[0], e, e32))
    assert e <= max(FACTOR * e32, FLOOR), (e, e32)
    assert (g == 7.0).all()


def test_row_bits_do_not_depend_on_the_instantiation(gpu):
    """row 1 of states_2481 (three labels) alone runs on the NJ = 1 kernel, in the batch on the NJ = 0 kernel: the same bits, as the
    kernel's header promises"""
    c = _case("states_2481")
    assert _alpha_beta_path(max(len(r) for r in c["labels"]))[1] == 0 and _alpha_beta_path(len(c["labels"][1]))[1] == 1
    p = _with_nan_tail(c)
    loss, grad = _run(gpu, p, c["labels"], c["lens"], c["blank"])
    loss1, grad1 = _run(gpu, p[1:], c["labels"][1:], c["lens"][1:], c["blank"])
    assert torch.isfinite(loss1).all() and torch.equal(loss1, loss[1:]) and torch.equal(grad1, grad[1:])


def _greedy_numpy(p, lens, blank):
    B, T, _ = p.shape
    out, n = np.full((B, T), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        prev = -1
        for t in range(lens[b]):
            k = int(np.argmax(p[b, t]))                 # first maximum = lowest index
            if k != prev and k != blank:
                out[b, n[b]] = k
                n[b] += 1
            prev = k
    return out, n


def _posteriors(rng, paths, T, Cc):
    p = rng.uniform(0.0, 0.1, (len(paths), T, Cc)).astype(np.float32)
    for b, path in enumerate(paths):
        for t, k in enumerate(path):
            p[b, t, k] = 0.5 + 0.01 * ((t * 7 + b) % 9)
    return p


def test_greedy_decode(gpu):
    """case 8: runs of repeats, repeats separated by a blank, leading and trailing blanks, an exact tie, lengths that include 0"""
    rng = np.random.default_rng(8)
    T, Cc, blank = 50, 7, 2
    base = [2, 2, 1, 1, 1, 2, 1, 3, 3, 2, 2, 3, 4, 4, 4, 4, 5, 2, 5, 5, 6, 0, 0, 2, 0, 1, 6, 6, 2, 2]
    paths = [(base + base)[:T], [int(k) for k in rng.integers(0, Cc, T)], (base[::-1] + base)[:T], [blank] * T, (base + base)[3:3 + T]]
    paths = [q + [blank] * (T - len(q)) for q in paths]
    lens = [50, 37, 0, 50, 41]
    p = _posteriors(rng, paths, T, Cc)
    p[0, 12, :] = 0.0; p[0, 12, 4] = 0.75; p[0, 12, 6] = 0.75; p[0, 12, 5] = 0.75          # an exact tie: class 4 wins
    p[4, 5, :] = 0.125                                                                       # ... and a whole frame tied: class 0
    want, wn = _greedy_numpy(p, lens, blank)
    assert wn[0] > 10 and wn[2] == 0 and wn[3] == 0
    out, n = NL.ctc_greedy_decode_device(torch.from_numpy(p).to(gpu), lens, blank)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(n.cpu().numpy(), wn)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    # more than one 256-frame chunk per row, C = 1000
    T2, C2 = 300, 1000
    path = [int(k) for k in np.repeat(rng.integers(0, C2, T2 // 3), 3)]
    p2 = _posteriors(rng, [path], T2, C2)
    want2, wn2 = _greedy_numpy(p2, [T2], 0)
    out2, n2 = NL.ctc_greedy_decode_device(torch.from_numpy(p2).to(gpu), None, 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(n2.cpu().numpy(), wn2)
    np.testing.assert_array_equal(out2.cpu().numpy(), want2)


def test_greedy_decode_past_the_grid(gpu):
    """more frames than the capped argmax grid covers in one trip: the grid-stride loop, across rows of lengths T, 0 and T - 1"""
    rng = np.random.default_rng(66000)
    B, T, Cc, blank = 3, 22000, 3, 1
    lens = [22000, 0, 21999]
    assert B * T == 66000 > ARGMAX_MAX_GRID * ARGMAX_FRAMES == 65536
    paths = []
    for b in range(B):
        path = np.repeat(rng.integers(0, Cc, T), rng.integers(1, 6, T))[:T]                  # runs of 1..5 equal frames
        for i, m in enumerate(range(256, T - 2, 256)):                                       # at the compaction's 256-frame chunk ends:
            k = (0, 2)[(i + b) % 2]
            if i % 3 == 0:
                path[m - 2:m + 2] = k                                                        # a run that straddles the boundary: one label
            elif i % 3 == 1:
                path[m - 1], path[m], path[m + 1] = k, blank, k                              # a blank on the boundary: the class twice
            else:
                path[m - 2:m], path[m:m + 2] = k, blank                                      # a run that ends with the chunk
        paths.append([int(k) for k in path])
    p = _posteriors(rng, paths, T, Cc)
    want, wn = _greedy_numpy(p, lens, blank)
    assert wn[0] > 2000 and wn[1] == 0 and wn[2] > 2000
    out, n = NL.ctc_greedy_decode_device(torch.from_numpy(p).to(gpu), lens, blank)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(n.cpu().numpy(), wn)
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_end_to_end_through_the_softmax_layer_gradient(gpu):
    """case 9: forward -> nntk_ctc_loss_device -> TimeDistributedDenseCalculateGradientDevice against float64 autograd of
    ctc_loss(log_softmax(x W + b)) summed over the rows: d_dprobs is what the softmax layer's gradient call takes, and padded frames
    contribute nothing"""
    L = capi.load()
    rng = np.random.default_rng(9)
    B, T, n_in, n_out, blank = 3, 20, 16, 9, 0
    lens, labels = [20, 13, 17], [[1, 2, 2, 5, 8], [3, 3, 4], [7, 1, 7, 1, 6, 2]]
    x = rng.uniform(-1, 1, (B, T, n_in)).astype(np.float32)
    W, bias = rng.uniform(-0.5, 0.5, (n_in, n_out)).astype(np.float32), rng.uniform(-0.1, 0.1, n_out).astype(np.float32)
    ah = L.ActivationFunctionCreateSoftmax(1, n_out)
    cfg = L.TimeDistributedDenseConfigCreate(T, L.DenseConfigCreate(n_in, n_out, ah))
    h = L.TimeDistributedDenseCreateForTraining(cfg, capi.ConvTrainingConfig(B))
    w = L.TimeDistributedDenseGetWeights(h).contents
    C.memmove(w.W, W.ctypes.data, W.nbytes); C.memmove(w.b, bias.ctypes.data, bias.nbytes)
    dp = lambda t: C.c_void_p(t.data_ptr())
    dx, probs = torch.from_numpy(x).to(gpu), torch.empty((B, T, n_out), device=gpu)
    assert L.TimeDistributedDenseApplyTrainingBatchDevice(h, dp(dx), dp(probs)) == 0, capi.last_error()
    loss, dprobs = NL.ctc_loss_device(probs, labels, input_lengths=lens, blank=blank)
    gwb, gx = torch.zeros(n_in * n_out + n_out, device=gpu), torch.empty_like(dx)
    assert L.TimeDistributedDenseCalculateGradientDevice(h, dp(gwb), dp(gx), dp(dprobs)) == 0, capi.last_error()
    torch.cuda.synchronize()

    def ref(dtype):
        xt = torch.from_numpy(x).to(dtype)
        Wt, bt = torch.from_numpy(W).to(dtype).requires_grad_(True), torch.from_numpy(bias).to(dtype).requires_grad_(True)
        lp = torch.log_softmax(xt @ Wt + bt, -1).transpose(0, 1)
        tgt = torch.zeros((B, 6), dtype=torch.long)
        for b_, r in enumerate(labels):
            tgt[b_, :len(r)] = torch.tensor(r)
        l = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor(lens), torch.tensor([len(r) for r in labels]), blank=blank, reduction="none")
        gW, gb = torch.autograd.grad(l.sum(), (Wt, bt))
        return l.detach().double().numpy(), gW.double().numpy(), gb.double().numpy()

    l64, W64, b64 = ref(torch.float64)
    l32, W32, b32 = ref(torch.float32)
    got = gwb.cpu().double().numpy()
    for nm, g, r64, r32 in (("d_W", got[:n_in * n_out].reshape(n_in, n_out), W64, W32), ("d_b", got[n_in * n_out:], b64, b32)):
        sc = np.abs(r64).max()
        e, e32 = np.abs(g - r64).max() / sc, np.abs(r32 - r64).max() / sc
        print("end to end %s: err %.2e, torch f32 err %.2e" % (nm, e, e32))
        assert e <= max(FACTOR * e32, FLOOR), (nm, e, e32)
    np.testing.assert_allclose(loss.cpu().double().numpy(), l64, rtol=1e-5)              # (the softmax itself is the layer's, in float32)
    L.TimeDistributedDenseDestroy(h); L.ActivationFunctionDestroy(ah)


def test_host_forms_equal_the_device_forms(gpu):
    c = _case("odd_C37")
    p = c["probs"]
    loss, grad = _run(gpu, p, c["labels"], c["lens"], c["blank"])
    hl, hg = NL.ctc_loss(p, c["labels"], input_lengths=c["lens"], blank=c["blank"])
    assert np.array_equal(hl, loss.numpy()) and np.array_equal(hg, grad.numpy())
    hl2, none = NL.ctc_loss(p, c["labels"], input_lengths=c["lens"], blank=c["blank"], want_grad=False)
    assert none is None and np.array_equal(hl2, hl)
    out, n = NL.ctc_greedy_decode_device(torch.from_numpy(p).to(gpu), c["lens"], c["blank"])
    torch.cuda.synchronize()
    ho, hn = NL.ctc_greedy_decode(p, c["lens"], c["blank"])
    assert np.array_equal(ho, out.cpu().numpy()) and np.array_equal(hn, n.cpu().numpy())
