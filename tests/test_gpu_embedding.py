"""The label embedding on the device (csrc/hip/rnnt_pred.hip): the lookup is bit copies of table rows, the table gradient is the sum of
each id's rows within the bound that follows from its summation alone, and its bits are a function of an id's own ascending row list.

The gradient's bound is derived, not tuned: an id with n occurrences is summed with n - 1 float32 additions whatever their shape, so per
element |err| <= (n - 1) 2^-24 sum |terms| (the standard first-order bound of recursive summation, which chunking only tightens); the
reference is the float64 sum of the same float32 rows, whose own error (2^-53 relative) is nine orders below."""
import numpy as np
import pytest
import torch

from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu


def _t(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.mark.parametrize("E", [1, 5, 64, 257, 1024])
@pytest.mark.parametrize("V", [2, 37])
@pytest.mark.parametrize("rows", [0, 1, 131])
def test_lookup_is_bit_exact(gpu, E, V, rows):
    rng = np.random.default_rng(1000 * E + 10 * V + rows)
    table = rng.standard_normal((V, E)).astype(np.float32)
    unused = V - 1
    table[unused] = np.nan                                                  # a row that no id names may hold NaN
    ids = rng.integers(0, V - 1, rows).astype(np.int32)
    ids[rng.random(rows) < 0.2] = -1
    want = np.where((ids >= 0)[:, None], table[np.maximum(ids, 0)], np.float32(0)).reshape(rows, E)
    d_table = _t(gpu, table)
    got = NL.embedding_lookup_device(d_table, ids)
    base = torch.full((rows * E + 1,), 7.0, device=gpu)                     # an output that is only 4-byte aligned
    off = NL.embedding_lookup_device(d_table, ids, out=base[1:].view(rows, E))
    assert rows == 0 or off.data_ptr() % 16 == 4
    torch.cuda.synchronize()
    assert torch.equal(got, _t(gpu, want)) and torch.equal(off, _t(gpu, want))
    assert float(base[0]) == 7.0
    assert not np.isnan(got.cpu().numpy()).any() and (got.cpu().numpy()[ids < 0] == 0).all()


def _dout(rng, rows, E):
    """mixed sign, magnitudes from 1e-3 to 1e3"""
    return (rng.choice([-1.0, 1.0], (rows, E)) * 10.0 ** rng.uniform(-3, 3, (rows, E))).astype(np.float32)


def _check_gradient(gpu, dout, ids, V, what):
    rows, E = dout.shape
    got = NL.embedding_gradient_device(_t(gpu, dout), ids, V)
    again = NL.embedding_gradient_device(_t(gpu, dout), ids, V)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two calls differ"
    got = got.cpu().numpy()
    worst = 0.0
    for v in range(V):
        r = np.flatnonzero(ids == v)
        if r.size == 0:
            assert (got[v] == 0).all() and not np.signbit(got[v]).any(), (what, v)
            continue
        if r.size == 1:
            assert np.array_equal(got[v].view(np.int32), dout[r[0]].view(np.int32)), (what, v)      # a bit copy
            continue
        terms = dout[r].astype(np.float64)
        err = np.abs(got[v].astype(np.float64) - terms.sum(0))
        bound = (r.size - 1) * 2.0 ** -24 * np.abs(terms).sum(0)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, v, r.size, ratio)
    print("%s: largest error / bound %.4f" % (what, worst))
    return got


COUNTS = {1: 1, 2: 2, 3: 33, 4: 64, 5: 65, 6: 300, 7: 7}                    # id 0 is absent; 33, 64, 65, 300 cross the 32-row chunk


@pytest.mark.parametrize("E", [1, 5, 64, 257, 1024])
def test_gradient_is_within_the_derived_bound(gpu, E):
    rng = np.random.default_rng(E)
    ids = np.concatenate([np.full(n, v, np.int32) for v, n in COUNTS.items()] + [np.full(40, -1, np.int32)])
    rng.shuffle(ids)
    dout = _dout(rng, ids.shape[0], E)
    dout[ids < 0] = np.nan                                                  # padding rows are never read
    got = _check_gradient(gpu, dout, ids, 8, "V = 8, E = %d" % E)
    assert np.isfinite(got).all()


def test_gradient_of_nothing_but_padding_and_of_no_rows(gpu):
    ids = np.full(50, -1, np.int32)
    dout = np.full((50, 12), np.nan, np.float32)
    got = _check_gradient(gpu, dout, ids, 8, "every row -1")
    assert (got == 0).all()
    dt = torch.full((8, 12), 7.0, device=gpu)
    NL.embedding_gradient_device(torch.empty((0, 12), device=gpu), np.zeros(0, np.int32), 8, dtable=dt)
    torch.cuda.synchronize()
    assert (dt == 0).all()


def test_gradient_on_tensors_that_are_only_4_byte_aligned(gpu):
    """the scalar path at a width the vector path would take: the same bits"""
    rng = np.random.default_rng(5)
    ids = rng.integers(-1, 8, 400).astype(np.int32)
    dout = _dout(rng, 400, 64)
    want = NL.embedding_gradient_device(_t(gpu, dout), ids, 8)
    base = torch.empty(400 * 64 + 1, device=gpu)
    shifted = base[1:].view(400, 64)
    shifted.copy_(_t(gpu, dout))
    tb = torch.empty(8 * 64 + 1, device=gpu)
    got = NL.embedding_gradient_device(shifted, ids, 8, dtable=tb[1:].view(8, 64))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_an_ids_bits_depend_on_its_own_rows_alone(gpu):
    """one id's gradient row: the same bits after the OTHER ids' rows are permuted, V goes from 8 to 4096, and the id's own rows move to
    other absolute positions in the same order"""
    rng = np.random.default_rng(77)
    E, K, rows = 40, 100, 400
    own = _dout(rng, K, E)
    outs = []
    for V, seed in ((8, 1), (8, 2), (4096, 3)):
        r2 = np.random.default_rng(seed)
        pos = np.sort(r2.choice(rows, K, replace=False))                    # the id's rows, in the same order at other positions
        ids = r2.integers(0, V, rows).astype(np.int32)
        ids[ids == 3] = 4
        ids[r2.random(rows) < 0.1] = -1
        ids[pos] = 3
        dout = _dout(r2, rows, E)                                           # the other ids' rows: other values, other places
        dout[pos] = own
        got = NL.embedding_gradient_device(_t(gpu, dout), ids, V)
        torch.cuda.synchronize()
        outs.append(got[3].cpu().numpy().view(np.int32).copy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_a_live_call_refuses_a_small_workspace_through_the_wrapper(gpu):
    ids = np.zeros(64, np.int32)
    with pytest.raises(AssertionError):
        NL.embedding_gradient_device(torch.zeros((64, 8), device=gpu), ids, 4, workspace=torch.empty(8, device=gpu))
    need = capi.load().nntk_embedding_workspace_floats(64, 4, 8)
    got = NL.embedding_gradient_device(torch.ones((64, 8), device=gpu), ids, 4, workspace=torch.empty(need, device=gpu))
    torch.cuda.synchronize()
    assert (got[0] == 64).all() and (got[1:] == 0).all()
