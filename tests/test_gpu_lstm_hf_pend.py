"""The HF instantiations of the register-resident LSTM (csrc/hip/recurrent_rr.hip, 256 < H <= 512: the recurrence on two f16 images of h, the
hand-off IS the FRAG2H output) with the hand-off by PENDING PATTERN (lstm_rr_hfp_kernel, option rec_hf_pend = 1, the default) against the
same instantiations with the flag words (rec_hf_pend = 0).  The two differ in how a consumer learns that a block is there, in no product
and in no summation order: every comparison here is bit for bit.

Shapes: ragged last tile and half, KX = 1 / 2 / 4, the smallest HF width (272), T just past the two preset timesteps.  The KX = 4 shapes
(in > 128) have no pending-pattern instantiation (it does not fit the register file): both option values run the flag kernel there, and
the comparisons hold trivially.
The reported kernel name is the family's for the default protocol and carries "flags" ahead of the ",hf>" suffix for the control.
(conftest.py does not know rec_hf_pend: every test here puts the option back itself.)
"""
import numpy as np
import pytest

from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

SHAPES = [(64, 5, 128, 272), (96, 17, 128, 512), (70, 40, 64, 384), (33, 3, 256, 512)]      # (B, T, in, H)
N_DENSE = 128


def u(r, *shape, sc=1.0):
    return r.uniform(-sc, sc, shape).astype(np.float32)


class Case:
    """one layer pair and two inputs per shape, built once per test"""

    def __init__(self, B, T, I, H, seed=0, dense=False):
        import torch
        r = np.random.default_rng(1000 * H + 10 * I + T + seed)
        self.B, self.T, self.I, self.H = B, T, I, H
        self.W, self.U, self.bi, self.bh = u(r, I, 4 * H, sc=I ** -0.5), u(r, H, 4 * H, sc=H ** -0.5), u(r, 4 * H, sc=0.1), u(r, 4 * H, sc=0.1)
        self.lstm = NL.LSTM(I, H, True, T, v2=True)
        self.lstm.set_weights(self.W, self.U, self.bi, self.bh)
        self.xa, self.xb = torch.from_numpy(u(r, B, T, I)).cuda(), torch.from_numpy(u(r, B, T, I)).cuda()
        self.tdd = None
        if dense:
            self.tdd = NL.TimeDistributedDense(T, H, N_DENSE)
            self.tdd.set_weights(u(r, H, N_DENSE, sc=H ** -0.5), u(r, N_DENSE, sc=0.1))

    def run(self, pend, x, out_h2=None):
        """the FRAG2H tensor as int32 words, and the name of the kernel that wrote it"""
        capi.set_option("rec_hf_pend", pend)
        try:
            h2 = NL.lstm_apply_device_frag2h(self.lstm, x=x, out_h2=out_h2)
            name = capi.load().nntk_hip_last_recurrent_kernel().decode()
        finally:
            capi.set_option("rec_hf_pend", "auto")
        assert name.startswith("lstm_rr_kernel<8,") and name.endswith(",hf>"), name
        assert ("flags" in name) == (pend == 0 and self.I <= 128), name       # (in > 128, KX = 4: the flag protocol only, one name)
        return h2, name

    def fused(self, pend, x):
        capi.set_option("rec_hf_pend", pend)
        try:
            return NL.lstm_tdd_apply_device(self.lstm, self.tdd, x).clone()
        finally:
            capi.set_option("rec_hf_pend", "auto")

    def close(self):
        self.lstm.destroy()
        if self.tdd:
            self.tdd.destroy()


def words(h2, B, T, H):
    """FRAG2H [T][2 ceil(B / 64)][H / 16][2] blocks of 64 lanes x 4 words -> the words of the rows < B (lane l of a block: row l & 31 of
    its half-tile), as one flat int32 tensor"""
    import torch
    nht = 2 * ((B + 63) // 64)
    w = h2.view(torch.int32).view(T, nht, H // 16, 2, 64, 4)
    row = torch.arange(nht, device=h2.device).view(nht, 1) * 32 + (torch.arange(64, device=h2.device) & 31).view(1, 64)
    return w.permute(1, 4, 0, 2, 3, 5)[row < B]


def same(c, a, b):
    import torch
    return torch.equal(words(a, c.B, c.T, c.H), words(b, c.B, c.T, c.H))


def status_ok():
    return capi.load().nntk_hip_device_status() == 0


@pytest.mark.parametrize("B,T,I,H", SHAPES)
def test_hf_pend_equals_the_flag_kernel_bit_for_bit(gpu, B, T, I, H):
    """The whole FRAG2H tensor (rows < B) and the fused LSTM -> dense output: equality, nothing less -- products and order are the same."""
    import torch
    c = Case(B, T, I, H, dense=True)
    flag, _ = c.run(0, c.xa)
    flag = flag.clone()
    pend, name = c.run(1, c.xa)
    assert name == "lstm_rr_kernel<8,%d,hf>" % (1 if I <= 64 else 2 if I <= 128 else 4)
    assert same(c, pend, flag)
    assert torch.isfinite(NL.frag2h_unpack_device(pend, B, T, H)).all()
    assert torch.equal(c.fused(1, c.xa), c.fused(0, c.xa))
    assert status_ok()
    c.close()


@pytest.mark.parametrize("B,T,I,H", SHAPES)
def test_hf_pend_never_takes_stale_or_preset_blocks_for_data(gpu, B, T, I, H):
    """Two different inputs alternate into ONE output tensor (a stale block of the launch before looks like data); then the tensor starts
    out full of plausible finite f16 values, then full of the pending pattern itself.  Every run equals the flag kernel's."""
    import torch
    c = Case(B, T, I, H)
    want_a, want_b = c.run(0, c.xa)[0].clone(), c.run(0, c.xb)[0].clone()
    out = torch.empty_like(want_a)
    for _ in range(2):
        assert same(c, c.run(1, c.xa, out_h2=out)[0], want_a)
        assert same(c, c.run(1, c.xb, out_h2=out)[0], want_b)
    out.view(torch.int16).fill_(0x3555)                       # f16 0.333 in every position, the two preset timesteps included
    assert same(c, c.run(1, c.xa, out_h2=out)[0], want_a)
    out.view(torch.int32).fill_(-1)                           # every block "not written"
    assert same(c, c.run(1, c.xb, out_h2=out)[0], want_b)
    assert status_ok()
    c.close()


def test_hf_pend_nan_propagates_as_in_the_flag_kernel_and_terminates(gpu):
    """A NaN in the input makes NaN h in one row from the first step on: NaN pairs are published, and a published NaN pair must never read
    as pending (the publisher's clamp).  The launch ends without the fault word, with NaNs where the flag kernel has them and the same values
    elsewhere.  Then one NaN weight: the host sends a layer with a non-finite weight to the exact kernels (the images cannot hold it), under
    either value of the option -- same output, and it terminates."""
    import torch
    B, T, I, H = SHAPES[1]
    c = Case(B, T, I, H, seed=5)
    x = c.xa.clone()
    x[5, 0, 7] = float("nan")
    flag = NL.frag2h_unpack_device(c.run(0, x)[0], B, T, H).clone()
    pend = NL.frag2h_unpack_device(c.run(1, x)[0], B, T, H)
    assert status_ok()
    assert torch.isnan(flag[5]).all() and not torch.isnan(flag[:5]).any() and not torch.isnan(flag[6:]).any()
    assert torch.equal(torch.isnan(pend), torch.isnan(flag))
    assert torch.equal(torch.nan_to_num(pend, nan=7.0), torch.nan_to_num(flag, nan=7.0))
    c.U[3, 17] = np.nan
    c.lstm.destroy()
    c.lstm = NL.LSTM(I, H, True, T, v2=True)                  # (a fresh layer: the weights go up once, with the NaN in them)
    c.lstm.set_weights(c.W, c.U, c.bi, c.bh)
    outs = []
    for opt in (0, 1):
        capi.set_option("rec_hf_pend", opt)
        try:
            outs.append(NL.frag2h_unpack_device(NL.lstm_apply_device_frag2h(c.lstm, x=c.xa), B, T, H).clone())
        finally:
            capi.set_option("rec_hf_pend", "auto")
    assert status_ok()
    assert torch.isnan(outs[0]).any()
    assert torch.equal(torch.isnan(outs[1]), torch.isnan(outs[0]))
    assert torch.equal(torch.nan_to_num(outs[1], nan=7.0), torch.nan_to_num(outs[0], nan=7.0))
    c.close()


def test_hf_pend_repeats_and_shards_equal_the_whole_batch(gpu):
    """Ten launches in one process give the first one's bits; a 64-row shard gives the bits of the same rows of the whole batch."""
    import torch
    B, T, I, H = SHAPES[1]
    c = Case(B, T, I, H, seed=9)
    first = c.run(1, c.xa)[0].clone()
    for _ in range(9):
        assert same(c, c.run(1, c.xa)[0], first)
    whole = NL.frag2h_unpack_device(first, B, T, H)
    xs = c.xa[32:].contiguous()
    shard = c.run(1, xs)[0].clone()
    assert torch.equal(NL.frag2h_unpack_device(shard, 64, T, H), whole[32:])
    assert torch.equal(words(shard, 64, T, H), words(c.run(0, xs)[0], 64, T, H))
    assert status_ok()
    c.close()


def test_carried_state_does_not_depend_on_the_hand_off_option(gpu):
    """The HF instantiations start from the zero state: a call that carries h_0 / c_0 in runs the bf16 x 3 kernels under either value of the
    option, and gives the same bits."""
    import torch
    B, T, I, H = 70, 6, 64, 384
    c = Case(B, T, I, H, seed=3)
    r = np.random.default_rng(4)
    h0, c0 = torch.from_numpy(u(r, B, H, sc=0.5)).cuda(), torch.from_numpy(u(r, B, H, sc=0.5)).cuda()
    outs = []
    for pend in (1, 0):
        capi.set_option("rec_hf_pend", pend)
        try:
            outs.append([t.clone() for t in c.lstm.apply_device_varlen(c.xa, None, h0=h0, c0=c0, return_state=True)])
        finally:
            capi.set_option("rec_hf_pend", "auto")
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0], c.lstm.apply_device(c.xa))       # (the state did go in)
    assert status_ok()
    c.close()
