"""Streaming CTC decoding (INTEGRATION.md "CTC prefix beam search", Streaming): a CtcBeamStream pushed chunk by chunk against the
one-shot nntk_ctc_beam_decode_device on the concatenated frames -- labels, lengths and the score bits, after every push -- and the
streaming best path against the one-shot best path.

"Equal" below is assert_array_equal on labels and lengths and on the scores viewed as int32.  The frames a push does not bring
(t >= n_frames[b]) are filled with NaN by the driver, so every case also checks that they influence nothing.

One case is anchored outside the kernels: the float64 prefix beam search of ctc_reference.py (dicts of label tuples, linear space, the
same candidate cells, merge order and canonical-index tie rule) under test_gpu_ctc_beam.py's premise -- at every frame
the relative gap between the W-th and the (W+1)-th candidate total, and between adjacent reported hypotheses, is at least
16 * T * 2^-24 -- and its score tolerance 8 * T * 2^-24 + 4 * ulp_f32(|ref|)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ctc_reference import chunk as _chunk, decode as _oneshot, drive as _drive, eq as _eq, reference, softmax as _softmax, tol as _tol
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu


def _frame_by_frame(lens):
    return [[1 if t < l else 0 for l in lens] for t in range(max(lens))]


def _largest(lens, mf):
    return [[min(mf, max(0, l - i * mf)) for l in lens] for i in range((max(lens) + mf - 1) // mf)]


# B = 3, T = 40, C = 9, W = 8, nbest = 3, blank = 8, rows of 40, 17 and 1 frames, at most 8 frames per push
CH = dict(B=3, T=40, C=9, W=8, nbest=3, blank=8, lens=[40, 17, 1], mf=8)
# rows advance by different amounts in one push, zero-frame pushes for single rows and for all of them
IRREGULAR = [[5, 0, 1], [0, 3, 0], [8, 0, 0], [0, 0, 0], [2, 8, 0], [7, 1, 0], [1, 5, 0], [8, 0, 0], [0, 0, 0], [8, 0, 0], [1, 0, 0]]


@functools.lru_cache(maxsize=None)
def _ch_probs():
    return _softmax(0, CH["B"], CH["T"], CH["C"])


@pytest.mark.parametrize("schedule", ["frame_by_frame", "irregular", "largest"])
def test_every_chunking_gives_the_one_shot_bits(gpu, schedule):
    """case 1"""
    c, p = CH, _ch_probs()
    pushes = dict(frame_by_frame=_frame_by_frame(c["lens"]), irregular=IRREGULAR, largest=_largest(c["lens"], c["mf"]))[schedule]
    assert [sum(n[b] for n in pushes) for b in range(c["B"])] == c["lens"]
    want = _oneshot(gpu, p, c["lens"], c["blank"], c["W"], 0, c["nbest"])
    dec = NL.CtcBeamStream(c["B"], c["mf"], c["C"], c["blank"], c["W"], 0, c["nbest"], max_labels=c["T"])
    _eq(_drive(gpu, dec, p, pushes, c["mf"]), want, schedule)
    dec.close()


def test_partial_results_after_every_push(gpu):
    """case 2: after every push the outputs are the one-shot call's on the frames seen so far"""
    c, p = CH, _ch_probs()
    dec = NL.CtcBeamStream(c["B"], c["mf"], c["C"], c["blank"], c["W"], 0, c["nbest"], max_labels=c["T"])

    def after(i, seen, got):
        _eq(got, _oneshot(gpu, p, seen, c["blank"], c["W"], 0, c["nbest"]), "push %d, frames seen %s" % (i, seen))

    _drive(gpu, dec, p, IRREGULAR, c["mf"], after=after)
    dec.close()


# name: (seed, B, T, C, W, cutoff, nbest, blank, lengths): the shapes of test_gpu_ctc_beam.py's PARITY that select the kernel's other
# instantiations (class_cut with T shortened to 12), and the full beam width
PATHS = {
    "class_cut": (0, 2, 12, 300, 8, 6, 2, 299, None),
    "unstaged": (0, 1, 8, 12000, 1, 0, 1, 11999, None),
    "unstaged_cut": (0, 1, 8, 9000, 2, 8000, 2, 8999, None),
    "staged_wide": (0, 2, 8, 2000, 4, 0, 2, 1999, [8, 5]),
    "staged_wide_cut": (0, 1, 8, 3000, 4, 1500, 2, 2999, None),
    "full_width": (1, 2, 24, 40, 128, 0, 8, 39, None),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_every_kernel_path_split_in_three(gpu, name):
    """case 3: 3 frames, no frame, the rest"""
    seed, B, T, Cc, W, cutoff, nbest, blank, lens = PATHS[name]
    lens = [T] * B if lens is None else lens
    p = _softmax(seed, B, T, Cc)
    want = _oneshot(gpu, p, lens, blank, W, cutoff, nbest)
    mf = T - 3
    dec = NL.CtcBeamStream(B, mf, Cc, blank, W, cutoff, nbest, max_labels=T)
    _eq(_drive(gpu, dec, p, [[3] * B, [0] * B, [l - 3 for l in lens]], mf), want, name)
    dec.close()


def test_frame_by_frame_against_the_float64_search(gpu):
    """case 4: the `small` shape, one frame per push in a block of three, against a reference that shares no code with the kernels"""
    seed, B, T, Cc, W, cutoff, nbest, blank = 0, 2, 12, 5, 4, 0, 4, 4
    p = _softmax(seed, B, T, Cc)
    lab, n, sc, gap, _ = reference(p, [T] * B, blank, W, cutoff, nbest)
    print("smallest relative gap %.3g, premise %.3g" % (gap, 16 * T * 2.0 ** -24))
    assert gap >= 16 * T * 2.0 ** -24, "the premise does not hold for this seed"
    dec = NL.CtcBeamStream(B, 3, Cc, blank, W, cutoff, nbest, max_labels=T)
    got_lab, got_n, got_sc = _drive(gpu, dec, p, _frame_by_frame([T] * B), 3)
    dec.close()
    np.testing.assert_array_equal(got_n, n)
    np.testing.assert_array_equal(got_lab, lab)
    fin = np.isfinite(sc)
    np.testing.assert_array_equal(np.isneginf(got_sc), ~fin)
    err = np.abs(got_sc[fin].astype(np.float64) - sc[fin])
    print("largest score error %.3g of %.3g allowed" % (err.max(initial=0.0), _tol(T, sc[fin]).min(initial=np.inf)))
    assert (err <= _tol(T, sc[fin])).all()


def test_exact_ties_across_chunk_boundaries(gpu):
    """case 5: uniform posteriors, one frame per push: the canonical-index tie rule alone decides, at every boundary"""
    T, Cc, W, blank = 6, 5, 4, 4
    p = np.full((1, T, Cc), 0.2, np.float32)
    want = _oneshot(gpu, p, [T], blank, W, 0, 4)
    dec = NL.CtcBeamStream(1, 1, Cc, blank, W, 0, 4, max_labels=T)
    _eq(_drive(gpu, dec, p, _frame_by_frame([T]), 1), want)
    dec.close()


def test_a_dead_beam_stays_dead_until_reset(gpu):
    """case 6: an all-zero frame in row 0's second push"""
    B, T, Cc, W, nbest, blank, mf = 2, 8, 5, 4, 2, 4, 3
    p = _softmax(11, B, T, Cc)
    p[0, 4] = 0.0
    dec = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T)
    seen_dead = []

    def after(i, seen, got):
        _eq(got, _oneshot(gpu, p, seen, blank, W, 0, nbest), "push %d" % i)
        seen_dead.append(bool((got[1][0] == -1).all() and (got[0][0] == -1).all() and np.isneginf(got[2][0]).all()))

    pos = [0] * B
    _drive(gpu, dec, p, [[3, 3], [3, 0], [2, 3], [0, 2]], mf, pos=pos, after=after)
    assert seen_dead == [False, True, True, True]
    row1 = _oneshot(gpu, p, [0, T], blank, W, 0, nbest)
    # a new stream in row 0's slot; row 1 brings nothing and keeps its result
    q = _softmax(12, B, T, Cc)
    dec.reset([0])
    got = _drive(gpu, dec, q, [[3, 0], [3, 0], [2, 0]], mf)
    dec.close()
    fresh = _oneshot(gpu, q, [T, 0], blank, W, 0, nbest)
    for g, f, r in zip(got, fresh, row1):
        assert g[0].tobytes() == f[0].tobytes() and g[1].tobytes() == r[1].tobytes()


def test_final_starts_a_new_stream_in_the_slot(gpu):
    """case 7: row 1 is final after 8 frames and then decodes another utterance; rows 0 and 2 go on"""
    B, T, Cc, W, nbest, blank, mf = 3, 12, 6, 4, 2, 5, 4
    p, q = _softmax(21, B, T, Cc), _softmax(22, B, T, Cc)
    dec = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T)
    pos = [0] * B
    got = _drive(gpu, dec, p, [[4] * B, [4] * B], mf, pos=pos, finals=[None, [0, 1, 0]])
    _eq(got, _oneshot(gpu, p, [8] * B, blank, W, 0, nbest), "the final push")
    mixed = p.copy()
    mixed[1, 8:] = q[1, :4]                                 # row 1's next frames are the new utterance's first four
    got = _drive(gpu, dec, mixed, [[4] * B], mf, pos=pos)
    dec.close()
    old = _oneshot(gpu, p, [T] * B, blank, W, 0, nbest)
    new = _oneshot(gpu, q, [0, 4, 0], blank, W, 0, nbest)
    for g, o, w in zip(got, old, new):
        assert g[0].tobytes() == o[0].tobytes() and g[2].tobytes() == o[2].tobytes()
        assert g[1].tobytes() == w[1].tobytes()


def test_max_labels_cuts_the_strings_and_nothing_else(gpu):
    """case 8: twelve labels in twelve frames, stored in 3 and in 12 places"""
    T, Cc, W, nbest, blank, mf = 12, 5, 4, 3, 4, 4
    path = [0, 1, 2, 3] * 3
    p = np.full((1, T, Cc), 0.025, np.float32)
    p[0, np.arange(T), path] = 0.9
    want = _oneshot(gpu, p, [T], blank, W, 0, nbest)
    assert want[1][0, 0] >= 6
    outs = {}
    for cap in (3, 12):
        dec = NL.CtcBeamStream(1, mf, Cc, blank, W, 0, nbest, max_labels=cap)
        outs[cap] = _drive(gpu, dec, p, _largest([T], mf), mf)
        dec.close()
        assert outs[cap][0].shape == (1, nbest, cap)
    _eq(outs[12], want)
    np.testing.assert_array_equal(outs[3][1], outs[12][1])
    np.testing.assert_array_equal(outs[3][2].view(np.int32), outs[12][2].view(np.int32))
    np.testing.assert_array_equal(outs[3][0], outs[12][0][:, :, :3])
    short = outs[3][1][0] < 3                               # a hypothesis shorter than the capacity: -1 behind its labels
    for k in np.nonzero(short)[0]:
        assert (outs[3][0][0, k, max(outs[3][1][0, k], 0):] == -1).all()


def test_determinism_and_row_independence(gpu):
    """case 9: the same bits twice; row 0's bits whatever the other rows carry and however they are chunked"""
    c, p = CH, _ch_probs()
    runs = []
    for _ in range(2):
        dec = NL.CtcBeamStream(c["B"], c["mf"], c["C"], c["blank"], c["W"], 0, c["nbest"], max_labels=c["T"])
        trace = []
        _drive(gpu, dec, p, IRREGULAR, c["mf"], after=lambda i, seen, got: trace.append(got))
        dec.close()
        runs.append(trace)
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    other = _softmax(31, c["B"], c["T"], c["C"])
    other[0] = p[0]
    pushes = [[n[0], min(8, max(0, 40 - 8 * i)), 3 if i < 4 else 0] for i, n in enumerate(IRREGULAR)]
    dec = NL.CtcBeamStream(c["B"], c["mf"], c["C"], c["blank"], c["W"], 0, c["nbest"], max_labels=c["T"])
    trace = []
    _drive(gpu, dec, other, pushes, c["mf"], after=lambda i, seen, got: trace.append(got))
    dec.close()
    for a, b in zip(runs[0], trace):
        for x, y in zip(a, b):
            assert x[0].tobytes() == y[0].tobytes()


def test_a_refused_push_writes_nothing_and_keeps_the_state(gpu):
    """case 10"""
    L = capi.load()
    B, T, Cc, W, nbest, blank, mf = 2, 8, 5, 4, 2, 4, 4
    p = _softmax(41, B, T, Cc)
    want = _oneshot(gpu, p, [T] * B, blank, W, 0, nbest)
    dec = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T)
    _drive(gpu, dec, p, [[4, 4]], mf)
    x = torch.from_numpy(_chunk(p, [4, 4], [4, 4], mf)).to(gpu)
    lab = torch.full((B, nbest, T), 7, dtype=torch.int32, device=gpu)
    n = torch.full((B, nbest), 7, dtype=torch.int32, device=gpu)
    sc = torch.full((B, nbest), 7.0, device=gpu)
    dp = lambda t: C.c_void_p(t.data_ptr())
    ok = np.asarray([4, 4], np.int32)
    ints = lambda a: np.asarray(a, np.int32).ctypes.data_as(capi.ip)
    refused = [
        (dp(x), ints([-1, 4]), dp(lab), dp(n), dp(sc)),
        (dp(x), ints([4, mf + 1]), dp(lab), dp(n), dp(sc)),
        (None, ints(ok), dp(lab), dp(n), dp(sc)),
        (dp(x), None, dp(lab), dp(n), dp(sc)),
        (dp(x), ints(ok), None, dp(n), dp(sc)),
        (dp(x), ints(ok), dp(lab), None, dp(sc)),
        (dp(x), ints(ok), dp(lab), dp(n), None),
    ]
    for i, (xp, nf, a, b, c) in enumerate(refused):
        rc = L.nntk_ctc_beam_stream_push_device(dec.h, xp, nf, None, a, b, c)
        assert rc == -1 and capi.last_error() != "", i
        torch.cuda.synchronize()
        assert (lab == 7).all() and (n == 7).all() and (sc == 7.0).all(), i
    out = dec.push(x, ok)
    torch.cuda.synchronize()
    _eq(tuple(t.cpu().numpy() for t in out), want)
    dec.close()


def _greedy_stream(gpu, p, lens, pushes, mf, blank):
    """-> per row the concatenated chunk outputs, and prev after every push"""
    B = p.shape[0]
    prev = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    pos, rows, prevs = [0] * B, [[] for _ in range(B)], []
    for n in pushes:
        x = torch.from_numpy(_chunk(p, pos, n, mf)).to(gpu)
        lab, cnt = NL.ctc_greedy_decode_stream_device(x, n, prev, blank)
        torch.cuda.synchronize()
        lab, cnt = lab.cpu().numpy(), cnt.cpu().numpy()
        for b in range(B):
            assert 0 <= cnt[b] <= n[b] and (lab[b, cnt[b]:] == -1).all() and (lab[b, :cnt[b]] >= 0).all()
            rows[b].extend(lab[b, :cnt[b]].tolist())
            pos[b] += n[b]
        prevs.append(prev.cpu().numpy().copy())
    assert pos == list(lens)
    return rows, prevs


@pytest.mark.parametrize("kind", ["random", "peaked"])
def test_streaming_best_path_equals_the_one_shot_best_path(gpu, kind):
    """case 11: B 3, T 30, C 7, ragged; five frames per push, with zero-frame pushes for rows 1 and 2"""
    B, T, Cc, blank, mf = 3, 30, 7, 6, 5
    lens = [30, 19, 7]
    if kind == "random":
        p = _softmax(51, B, T, Cc)
    else:
        # boundaries at 5, 10, 15, ...: 4|5 two equal argmax frames; 9|10 a blank, then the label before it again; 14|15 a label,
        # then a blank and the label again; 19|20 two blanks; 24|25 two different labels
        row = [0, 1, 1, 6, 2, 2, 2, 0, 3, 6, 3, 3, 6, 6, 4, 6, 4, 5, 6, 6, 6, 6, 1, 0, 0, 5, 5, 6, 2, 2]
        paths = np.array([row, row[5:] + row[:5], row[10:] + row[:10]])
        p = np.full((B, T, Cc), 0.02, np.float32)
        np.put_along_axis(p, paths[:, :, None], 0.88, axis=2)
    pushes = [[5, 5, 5], [5, 0, 2], [5, 5, 0], [5, 5, 0], [5, 4, 0], [5, 0, 0]]
    rows, prevs = _greedy_stream(gpu, p, lens, pushes, mf, blank)
    want, wn = NL.ctc_greedy_decode_device(torch.from_numpy(p).to(gpu), lens, blank)
    torch.cuda.synchronize()
    want, wn = want.cpu().numpy(), wn.cpu().numpy()
    for b in range(B):
        assert rows[b] == want[b, :wn[b]].tolist(), b
    arg = p.argmax(-1)
    assert prevs[0].tolist() == [arg[0, 4], arg[1, 4], arg[2, 4]]
    assert prevs[1][1] == prevs[0][1] and prevs[2][2] == prevs[1][2]             # zero-frame rows keep theirs
    assert prevs[-1].tolist() == [arg[0, 29], arg[1, 18], arg[2, 6]]
    if kind == "peaked":
        assert rows[0] == [0, 1, 2, 0, 3, 3, 4, 4, 5, 1, 0, 5, 2]


def test_host_form_equals_the_device_form(gpu):
    """case 13"""
    c, p = CH, _ch_probs()
    dev = NL.CtcBeamStream(c["B"], c["mf"], c["C"], c["blank"], c["W"], 0, c["nbest"], max_labels=c["T"])
    host = NL.CtcBeamStream(c["B"], c["mf"], c["C"], c["blank"], c["W"], 0, c["nbest"], max_labels=c["T"])
    pos = [0] * c["B"]
    for n in IRREGULAR[:5]:
        x = _chunk(p, pos, n, c["mf"])
        a = dev.push(torch.from_numpy(x).to(gpu), n)
        torch.cuda.synchronize()
        b = host.push_host(x, n)
        for u, v in zip(a, b):
            assert u.cpu().numpy().tobytes() == v.tobytes()
        pos = [q + k for q, k in zip(pos, n)]
    dev.close()
    host.close()


def test_stack_into_beam_stream_equals_one_shot_chain_and_decode(gpu):
    """case 12: Spectrogram -> Conv1d + BN + ReLU -> RNN-192 -> TimeDistributedDense -> softmax (the smallest stack of
    test_gpu_stream_stack.py, with a softmax head), pushed in chunks into a CtcBeamStream, against the one-shot chain followed by
    ctc_beam_decode_device"""
    from nntoolkitcore_amd.streaming import StreamingStack
    NFFT, WIN, NOV, CAP = 512, 400, 240, 2560
    rng = np.random.default_rng(8)
    u = lambda *s, sc=1.0: rng.uniform(-sc, sc, s).astype(np.float32)
    B, H, V, W, nbest, blank = 3, 192, 12, 8, 2, 0
    totals = [int(rng.integers(3000, 7000)) for _ in range(B)]
    streams = [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in totals]
    spec = NL.Spectrogram(NFFT, WIN, NOV, CAP)
    conv = NL.Conv1d(257, 128, 5, 1, spec.stream_sizes()[1])
    conv_w = (u(128, 257, 5, sc=(257 * 5) ** -0.5), u(128, sc=0.1))
    conv.set_weights(*conv_w)
    bn = NL.BatchNorm(128, 1e-3, 1)
    bn.set_weights(1 + u(128, sc=0.5), u(128, sc=0.5), u(128, sc=0.1), 1 + np.abs(u(128, sc=0.5)))
    relu = NL.Activation("relu", 1, 1.0)
    T = conv.stream_sizes()[1]
    rw = (u(128, H, sc=128 ** -0.5), u(H, H, sc=H ** -0.5), u(H, sc=0.1), u(H, sc=0.1))
    dw = (u(H, V, sc=4 * H ** -0.5), u(V, sc=0.1))
    soft = NL.Activation("softmax", 1, vector_size=V)
    rnn = NL.RNN(128, H, True, T, v2=True)
    rnn.set_weights(*rw)
    tdd = NL.TimeDistributedDense(T, H, V)
    tdd.set_weights(*dw)
    stack = StreamingStack(spec, [(conv, bn, relu)], [rnn], head=tdd, batch=B)

    # one-shot chain
    specs = []
    for s in streams:
        sp = NL.Spectrogram(NFFT, WIN, NOV, len(s))
        specs.append(sp.apply_device(torch.from_numpy(s[None]).cuda())[0])
        sp.destroy()
    Fm = max(t.shape[0] for t in specs)
    xp = torch.zeros((B, Fm, 257), device="cuda")
    for b, t in enumerate(specs):
        xp[b, :t.shape[0]] = t
    conv1 = NL.Conv1d(257, 128, 5, 1, Fm)
    conv1.set_weights(*conv_w)
    cc = conv1.apply_device(xp, bn=bn, act=relu)
    lens = np.array([max(0, t.shape[0] - 4) for t in specs], np.int32)
    Tm = cc.shape[1]
    r1 = NL.RNN(128, H, True, Tm, v2=True)
    r1.set_weights(*rw)
    d1 = NL.TimeDistributedDense(Tm, H, V)
    d1.set_weights(*dw)
    probs = soft.apply_device(d1.apply_device(r1.apply_device_varlen(cc, lens)), size=B * Tm)
    want = NL.ctc_beam_decode_device(probs, lens, blank, W, 0, nbest)
    torch.cuda.synchronize()
    want = tuple(t.cpu().numpy() for t in want)
    assert want[1][:, 0].min() >= 0

    dec = NL.CtcBeamStream(B, T, V, blank, W, 0, nbest, max_labels=Tm)
    pos, hop, got, result = [0] * B, [2560, 1000, 1700], None, [None] * B
    while any(pos[b] < totals[b] for b in range(B)):
        x = np.zeros((B, CAP), np.float32)
        n_new, final = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            n = min(hop[b], totals[b] - pos[b])
            x[b, :n] = streams[b][pos[b]:pos[b] + n]
            final[b] = int(n > 0 and pos[b] + n == totals[b])
            n_new[b] = n
            pos[b] += n
        out, cnt = stack.push(torch.from_numpy(x).cuda(), n_new, final)
        got = dec.push(soft.apply_device(out, size=B * T), cnt, final)
        torch.cuda.synchronize()
        for b in np.nonzero(final)[0]:
            result[b] = tuple(t.cpu().numpy()[b] for t in got)
    for b in range(B):
        for g, w in zip(result[b], want):
            assert g.tobytes() == w[b].tobytes(), b
    dec.close()
    for o in (spec, conv, bn, relu, rnn, tdd, conv1, r1, d1, soft):
        o.destroy()
