"""Thin Python mirror of the reference's layer protocol over the C boundary
(capi.py): ``XConfigCreate -> XCreateForInference -> XGetWeights (copy weights in)
-> XApply* -> XDestroy``.  Names and argument meaning follow the reference's C API
(conv_1d.h, batch_norm.h, gru.h, lstm.h, dense.h, time_distributed_dense.h,
spectrogram.h) so parity tests read like a C caller.  No arithmetic happens here.

``apply(np_array)`` uses the host-pointer C entry points; ``apply_device(tensor)``
passes torch-ROCm device pointers to the ``*ApplyDevice`` entry points (torch is
only the owner of HBM buffers and streams).
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, fp

ACT_IDENTITY, ACT_SIGMOID, ACT_TANH, ACT_RELU, ACT_SOFTMAX = "identity", "sigmoid", "tanh", "relu", "softmax"


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(fp)


def _fill(ptr, arr):
    arr = _f32(arr).ravel()
    C.memmove(ptr, arr.ctypes.data, arr.nbytes)


def _dp(t):
    """device pointer of a contiguous float32 torch tensor"""
    assert t.is_cuda and t.is_contiguous() and t.dtype.is_floating_point and t.element_size() == 4
    return C.c_void_p(t.data_ptr())


def _host_ints(a, B, what):
    """a host int32 array of B entries that the C call may read and write (in place when `a` already is one)"""
    if isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous and a.ndim == 1:
        assert a.shape[0] == B, what + ": one per row"
        return a
    v = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    assert v.shape[0] == B, what + ": one per row"
    return v


def _stream_call(fn, name, pre, x, row_shape, n_new, state, state_row, final, post_out, out):
    """shared driver of the *ApplyDeviceStream wrappers: state = (device state tensor, host int32 lengths) -- both updated in place.
    The C call reads [B][row_shape] input and [B][state_row] state and writes post_out: the tensors must be exactly that large."""
    B = x.shape[0]
    st, lens = state
    if tuple(x.shape[1:]) != tuple(row_shape):
        raise ValueError("%s: input rows must be %s (the handle's input_size), got %s" % (name, tuple(row_shape), tuple(x.shape[1:])))
    if tuple(st.shape) != (B,) + tuple(state_row) or not st.is_contiguous():
        raise ValueError("%s: state tensor must be contiguous %s, got %s" % (name, (B,) + tuple(state_row), tuple(st.shape)))
    if out is not None and (tuple(out.shape) != tuple(post_out) or not out.is_contiguous()):
        raise ValueError("%s: out must be contiguous %s, got %s" % (name, tuple(post_out), tuple(out.shape)))
    assert isinstance(lens, np.ndarray) and lens.dtype == np.int32 and lens.shape == (B,), "state: (tensor, int32 [B] lengths)"
    nn = _host_ints(n_new, B, "n_new")
    fin = None if final is None else _host_ints(np.asarray(final, dtype=np.int32), B, "final")
    counts = np.zeros(B, np.int32)
    if out is None:
        out = x.new_empty(post_out)
    check(fn(*pre, _dp(x), nn.ctypes.data_as(capi.ip), fin.ctypes.data_as(capi.ip) if fin is not None else None,
             _dp(st), lens.ctypes.data_as(capi.ip), _dp(out), counts.ctypes.data_as(capi.ip), B), name)
    return out, counts


def use_torch_stream():
    """Route every launch to torch's current HIP stream so torch events/timing see the kernels."""
    import torch
    capi.load().nntk_hip_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))


class Activation:
    def __init__(self, kind, size, a=1.0, vector_size=0):
        L = capi.load()
        self.kind, self.size, self.vector_size = kind, size, vector_size
        if kind == ACT_IDENTITY:
            self.h = L.ActivationFunctionCreateIdentity(size)
        elif kind == ACT_SIGMOID:
            self.h = L.ActivationFunctionCreateSigmoid(size)
        elif kind == ACT_TANH:
            self.h = L.ActivationFunctionCreateTanh(size)
        elif kind == ACT_RELU:
            self.h = L.ActivationFunctionCreateReLU(size, C.c_float(a))
        elif kind == ACT_SOFTMAX:
            self.h = L.ActivationFunctionCreateSoftmax(size, vector_size)
        else:
            raise ValueError(kind)

    def apply(self, x):
        x = _f32(x)
        out = np.empty_like(x)
        capi.load().ActivationFunctionApply(self.h, _p(x), _p(out))
        err = capi.last_error()
        if err:
            raise capi.NNTKError(err)
        return out

    def apply_device(self, x, out=None, size=0):
        out = x.new_empty(x.shape) if out is None else out
        check(capi.load().ActivationFunctionApplyDevice(self.h, _dp(x), _dp(out), size), "ActivationFunctionApplyDevice")
        return out

    def destroy(self):
        if self.h:
            capi.load().ActivationFunctionDestroy(self.h)
            self.h = None


class Conv1d:
    def __init__(self, cin, cout, k, stride, input_size):
        L = capi.load()
        self.cfg = L.Conv1dConfigCreate(cin, cout, k, stride, input_size)
        self.h = L.Conv1dCreateForInference(self.cfg)
        if not self.h:
            raise capi.NNTKError("Conv1dCreateForInference: " + capi.last_error())

    def set_weights(self, W, b):
        w = capi.load().Conv1dGetWeights(self.h).contents
        _fill(w.W, W)
        _fill(w.b, b)

    @property
    def out_shape(self):
        return (self.cfg.output_size, self.cfg.output_feature_channels)

    def apply(self, x):
        x = _f32(x)
        L = capi.load()
        if x.ndim == 2:
            out = np.empty(self.out_shape, np.float32)
            check(L.Conv1dApplyInference(self.h, _p(x), _p(out)), "Conv1dApplyInference")
        else:
            out = np.empty((x.shape[0],) + self.out_shape, np.float32)
            check(L.Conv1dApplyInferenceBatch(self.h, _p(x), _p(out), x.shape[0]), "Conv1dApplyInferenceBatch")
        return out

    def apply_device(self, x, out=None, bn=None, act=None):
        B = x.shape[0]
        if out is None:
            out = x.new_empty((B,) + self.out_shape)
        L = capi.load()
        if bn is None and act is None:
            check(L.Conv1dApplyDevice(self.h, _dp(x), _dp(out), B), "Conv1dApplyDevice")
        else:
            check(L.Conv1dBatchNormActivationApplyDevice(self.h, bn.h if bn else None, act.h if act else None,
                                                         _dp(x), _dp(out), B), "Conv1dBatchNormActivationApplyDevice")
        return out

    def stream_sizes(self):
        """(hist_rows, max_outputs): nntk_conv1d_stream_sizes"""
        a, b = C.c_int(), C.c_int()
        check(capi.load().nntk_conv1d_stream_sizes(self.cfg, C.byref(a), C.byref(b)), "nntk_conv1d_stream_sizes")
        return a.value, b.value

    def new_stream_state(self, batch):
        """(history [batch, k - 1, Cin] zeros on the current device, host int32 hist_len [batch] zeros)"""
        import torch
        hr, _ = self.stream_sizes()
        return (torch.zeros((batch, hr, self.cfg.input_feature_channels), device="cuda"), np.zeros(batch, np.int32))

    def apply_device_stream(self, x, n_new, state, bn=None, act=None, final=None, out=None):
        """Conv1dBatchNormActivationApplyDeviceStream: x [B, input_size, Cin] chunk rows, row b brings n_new[b] of them.
        Returns (out [B, max_outputs, Cout], n_out); the state (history tensor, hist_len) is updated in place."""
        hr, mo = self.stream_sizes()
        cin = self.cfg.input_feature_channels
        return _stream_call(capi.load().Conv1dBatchNormActivationApplyDeviceStream, "Conv1dBatchNormActivationApplyDeviceStream",
                            (self.h, bn.h if bn else None, act.h if act else None), x, (self.cfg.input_size, cin), n_new, state,
                            (hr, cin), final, (x.shape[0], mo, self.cfg.output_feature_channels), out)

    def apply_device_frag3(self, x, out_f3=None, bn=None, act=None):
        """Conv1dBatchNormActivationApplyDeviceFrag3: the (fused) layer output [B, Tout, Cout] as a frag3 buffer."""
        B = x.shape[0]
        L = capi.load()
        if out_f3 is None:
            out_f3 = x.new_empty(L.nntk_frag3_floats(B, *self.out_shape))
        check(L.Conv1dBatchNormActivationApplyDeviceFrag3(self.h, bn.h if bn else None, act.h if act else None,
                                                          _dp(x), _dp(out_f3), B), "Conv1dBatchNormActivationApplyDeviceFrag3")
        return out_f3

    def sync_weights(self):
        check(capi.load().Conv1dSyncWeights(self.h), "Conv1dSyncWeights")

    def load_weights_device(self, block):
        """Conv1dLoadWeightsDevice: the GetWeights() block from a device tensor (same order and size), then what sync_weights does"""
        check(capi.load().Conv1dLoadWeightsDevice(self.h, _dp(block)), "Conv1dLoadWeightsDevice")

    def destroy(self):
        if self.h:
            capi.load().Conv1dDestroy(self.h)
            self.h = None


class BatchNorm:
    def __init__(self, channels, epsilon, count):
        L = capi.load()
        self.cfg = L.BatchNormConfigCreate(channels, C.c_float(epsilon), count)
        self.h = L.BatchNormCreateForInference(self.cfg)

    def set_weights(self, gamma, beta, mean, var):
        w = capi.load().BatchNormGetWeights(self.h).contents
        _fill(w.gamma, gamma)
        _fill(w.beta, beta)
        _fill(w.moving_mean, mean)
        _fill(w.moving_variance, var)

    def apply(self, x):
        x = _f32(x)
        out = np.empty_like(x)
        check(capi.load().BatchNormApplyInference(self.h, _p(x), _p(out)), "BatchNormApplyInference")
        return out

    def apply_device(self, x, out=None):
        out = x.new_empty(x.shape) if out is None else out
        rows = x.numel() // self.cfg.feature_channels
        check(capi.load().BatchNormApplyDevice(self.h, _dp(x), _dp(out), rows), "BatchNormApplyDevice")
        return out

    def load_weights_device(self, block):
        """BatchNormLoadWeightsDevice: the GetWeights() block from a device tensor (same order and size), then what sync_weights does"""
        check(capi.load().BatchNormLoadWeightsDevice(self.h, _dp(block)), "BatchNormLoadWeightsDevice")

    def destroy(self):
        if self.h:
            capi.load().BatchNormDestroy(self.h)
            self.h = None


class _Recurrent:
    def set_weights(self, W, U, b_i, b_h):
        w = self._get_weights(self.h).contents
        _fill(w.W, W)
        _fill(w.U, U)
        _fill(w.b_i, b_i)
        _fill(w.b_h, b_h)

    def _out(self, x_shape_prefix, alloc):
        T, H = self.cfg.base.timesteps, self.cfg.base.output_feature_channels
        tail = (T, H) if self.cfg.base.return_sequences else (H,)
        return alloc(tuple(x_shape_prefix) + tail)

    def apply(self, x):
        x = _f32(x)
        if x.ndim == 2:     # one sequence, stateful
            out = self._out((), lambda s: np.empty(s, np.float32))
            check(self._apply(self.h, _p(x), _p(out)), type(self).__name__ + "ApplyInference")
        else:
            out = self._out((x.shape[0],), lambda s: np.empty(s, np.float32))
            check(self._apply_batch(self.h, _p(x), _p(out), x.shape[0]), type(self).__name__ + "ApplyInferenceBatch")
        return out

    def apply_device(self, x, out=None):
        if out is None:
            out = self._out((x.shape[0],), lambda s: x.new_empty(s))
        check(self._apply_device(self.h, _dp(x), _dp(out), x.shape[0]), type(self).__name__ + "ApplyDevice")
        return out

    def apply_device_varlen(self, x, lengths=None, h0=None, c0=None, return_state=False, out=None, hT=None, cT=None):
        """Ragged batch with carried state (``*ApplyDeviceVarLen``): x [B,T,in] device tensor, row b runs its first
        lengths[b] steps (None: all T) from h0[b] (c0[b], LSTM); sequence outputs past a row's length are zeros.
        Returns out, or (out, hT) / (out, hT, cT) with return_state (written into hT / cT when given)."""
        B = x.shape[0]
        H = self.cfg.base.output_feature_channels
        if out is None:
            out = self._out((B,), lambda s: x.new_empty(s))
        lp = None
        if lengths is not None:
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
            assert lens.shape[0] == B, "lengths: one per row"
            lp = lens.ctypes.data_as(capi.ip)
        nul = C.c_void_p(None)
        if return_state and hT is None:
            hT = x.new_empty((B, H))
        state_in = [h0] + ([c0] if self._is_lstm else [])
        state = [_dp(t) if t is not None else nul for t in state_in]
        if return_state and self._is_lstm and cT is None:
            cT = x.new_empty((B, H))
        state += [_dp(hT) if hT is not None else nul] + ([_dp(cT) if cT is not None else nul] if self._is_lstm else [])
        check(self._apply_device_vl(self.h, _dp(x), _dp(out), B, lp, *state), type(self).__name__ + "ApplyDeviceVarLen")
        if not return_state:
            return out
        return (out, hT, cT) if self._is_lstm else (out, hT)

    def sync_weights(self):
        check(self._sync(self.h), "SyncWeights")

    def load_weights_device(self, block):
        """<GRU|LSTM|RNN>LoadWeightsDevice: the block W | U | b_i | b_h from a device tensor, then what sync_weights does"""
        name = type(self).__name__ + "LoadWeightsDevice"
        check(getattr(capi.load(), name)(self.h, _dp(block)), name)

    def reset_state(self):
        check(self._reset(self.h), "ResetState")

    def destroy(self):
        if self.h:
            self._destroy(self.h)
            self._acts_destroy(self.acts)
            self.h = None


class GRU(_Recurrent):
    def __init__(self, in_features, hidden, return_sequences, timesteps, acts=None, mini_batch=None):
        L = capi.load()
        self.acts = L.GRUActivationsCreateDefault(hidden) if acts is None else acts
        self.cfg = L.GRUConfigCreate(in_features, hidden, return_sequences, timesteps, self.acts)
        # mini_batch: a *CreateForTraining handle of that mini-batch size (the training calls), else an inference handle
        self.mini_batch = mini_batch
        self.h = (L.GRUCreateForTraining(self.cfg, capi.ConvTrainingConfig(mini_batch)) if mini_batch else
                  L.GRUCreateForInference(self.cfg))
        self._get_weights, self._apply, self._apply_batch = L.GRUGetWeights, L.GRUApplyInference, L.GRUApplyInferenceBatch
        self._apply_device, self._sync, self._reset = L.GRUApplyDevice, L.GRUSyncWeights, L.GRUResetState
        self._apply_device_vl, self._is_lstm = L.GRUApplyDeviceVarLen, False
        self._destroy, self._acts_destroy = L.GRUDestroy, L.GRUActivationsDestroy

    def state(self):
        h = np.empty(self.cfg.base.output_feature_channels, np.float32)
        check(capi.load().GRUGetState(self.h, _p(h)), "GRUGetState")
        return h


def gru_stack2_apply_device(g1, g2, x, out=None):
    """GRUStack2ApplyDevice: two stacked GRU layers in one persistent launch (zero initial state)."""
    H, T = g2.cfg.base.output_feature_channels, g2.cfg.base.timesteps
    if out is None:
        out = x.new_empty((x.shape[0], T, H) if g2.cfg.base.return_sequences else (x.shape[0], H))
    check(capi.load().GRUStack2ApplyDevice(g1.h, g2.h, _dp(x), _dp(out), x.shape[0]), "GRUStack2ApplyDevice")
    return out


# ---- frag3 tensors (nntoolkitcore_hip.h: activations pre-split for the split-bf16 x 3 contraction, MFMA fragment order) ----

def frag3_pack_device(x):
    """[B, T, C] f32 device tensor -> its frag3 form (a flat f32-typed device buffer of nntk_frag3_floats(B, T, C) floats)."""
    B, T, Cc = x.shape
    L = capi.load()
    out = x.new_empty(L.nntk_frag3_floats(B, T, Cc))
    check(L.nntk_frag3_pack_device(_dp(x), _dp(out), B, T, Cc), "nntk_frag3_pack_device")
    return out


def frag3_unpack_device(f3, B, T, Cc):
    """frag3 buffer -> [B, T, C] f32 device tensor (exact: hi + mid + lo)."""
    out = f3.new_empty((B, T, Cc))
    check(capi.load().nntk_frag3_unpack_device(_dp(f3), _dp(out), B, T, Cc), "nntk_frag3_unpack_device")
    return out


def recurrent_apply_device_frag3(layer, x=None, x_f3=None, batch=None, want_f32=True, want_f3=False, out=None, out_f3=None):
    """<GRU|LSTM>ApplyDeviceFrag3: input as f32 `x` [B, T, in] or frag3 `x_f3` (then `batch` is required); returns (out_f32 | None,
    out_frag3 | None).  `out` / `out_f3`: preallocated outputs (they imply want_f32 / want_f3)."""
    L = capi.load()
    fn = L.LSTMApplyDeviceFrag3 if isinstance(layer, LSTM) else L.GRUApplyDeviceFrag3
    B = x.shape[0] if x is not None else batch
    src = x if x is not None else x_f3
    H, T = layer.cfg.base.output_feature_channels, layer.cfg.base.timesteps
    if out is None and want_f32:
        out = src.new_empty((B, T, H) if layer.cfg.base.return_sequences else (B, H))
    out3 = out_f3
    if out3 is None and want_f3:
        out3 = src.new_empty(L.nntk_frag3_floats(B, T, H))
    check(fn(layer.h, _dp(x) if x is not None else None, _dp(x_f3) if x_f3 is not None else None,
             _dp(out) if out is not None else None, _dp(out3) if out3 is not None else None, B), "ApplyDeviceFrag3")
    return out, out3


def tdd_apply_device_frag3(tdd, x_f3, batch, out=None):
    """TimeDistributedDenseApplyDeviceFrag3: the input [batch, ts, in] in frag3 form."""
    if out is None:
        out = x_f3.new_empty((batch, tdd.cfg.ts, tdd.cfg.dense.output_size))
    check(capi.load().TimeDistributedDenseApplyDeviceFrag3(tdd.h, _dp(x_f3), _dp(out), batch), "TimeDistributedDenseApplyDeviceFrag3")
    return out


# ---- frag2h tensors (nntoolkitcore_hip.h: a bounded activation tensor, |x| < 2, as two f16 images for the three-product contraction) ----

def frag2h_pack_device(x):
    """[B, T, C] f32 device tensor with |x| < 2 -> its frag2h form (a flat f32-typed device buffer of nntk_frag2h_floats(B, T, C) floats)."""
    B, T, Cc = x.shape
    L = capi.load()
    out = x.new_empty(L.nntk_frag2h_floats(B, T, Cc))
    check(L.nntk_frag2h_pack_device(_dp(x), _dp(out), B, T, Cc), "nntk_frag2h_pack_device")
    return out


def frag2h_unpack_device(h2, B, T, Cc):
    """frag2h buffer -> [B, T, C] f32 device tensor ((hi + lo) 2^-15: the value to 2^-23 relative at worst)."""
    out = h2.new_empty((B, T, Cc))
    check(capi.load().nntk_frag2h_unpack_device(_dp(h2), _dp(out), B, T, Cc), "nntk_frag2h_unpack_device")
    return out


def lstm_apply_device_frag2h(lstm, x=None, x_f3=None, batch=None, out_h2=None):
    """LSTMApplyDeviceFrag2h: input as f32 `x` [B, T, in] or frag3 `x_f3` (then `batch` is required); returns the sequence output in frag2h form."""
    L = capi.load()
    B = x.shape[0] if x is not None else batch
    src = x if x is not None else x_f3
    H, T = lstm.cfg.base.output_feature_channels, lstm.cfg.base.timesteps
    if out_h2 is None:
        out_h2 = src.new_empty(L.nntk_frag2h_floats(B, T, H))
    check(L.LSTMApplyDeviceFrag2h(lstm.h, _dp(x) if x is not None else None, _dp(x_f3) if x_f3 is not None else None, _dp(out_h2), B),
          "LSTMApplyDeviceFrag2h")
    return out_h2


def tdd_apply_device_frag2h(tdd, x_h2, batch, out=None):
    """TimeDistributedDenseApplyDeviceFrag2h: the input [batch, ts, in] in frag2h form."""
    if out is None:
        out = x_h2.new_empty((batch, tdd.cfg.ts, tdd.cfg.dense.output_size))
    check(capi.load().TimeDistributedDenseApplyDeviceFrag2h(tdd.h, _dp(x_h2), _dp(out), batch), "TimeDistributedDenseApplyDeviceFrag2h")
    return out


def lstm_tdd_apply_device(lstm, tdd, x, out=None):
    """LSTMTimeDistributedDenseApplyDevice: LSTM (return_sequences) -> TimeDistributedDense with the tensor in between in frag3 form."""
    if out is None:
        out = x.new_empty((x.shape[0], tdd.cfg.ts, tdd.cfg.dense.output_size))
    check(capi.load().LSTMTimeDistributedDenseApplyDevice(lstm.h, tdd.h, _dp(x), _dp(out), x.shape[0]), "LSTMTimeDistributedDenseApplyDevice")
    return out


def gru_stack2_apply(g1, g2, x):
    """GRUStack2ApplyInferenceBatch on host arrays [B, T, in]."""
    x = _f32(x)
    H, T = g2.cfg.base.output_feature_channels, g2.cfg.base.timesteps
    out = np.empty((x.shape[0], T, H) if g2.cfg.base.return_sequences else (x.shape[0], H), np.float32)
    check(capi.load().GRUStack2ApplyInferenceBatch(g1.h, g2.h, _p(x), _p(out), x.shape[0]), "GRUStack2ApplyInferenceBatch")
    return out


class RNN(_Recurrent):
    """One-gate recurrent layer (rnn.h); `act` is an ActivationFunction handle (default tanh over H)."""

    def __init__(self, in_features, hidden, return_sequences, timesteps, v2=True, act=None, mini_batch=None):
        L = capi.load()
        self.act = L.ActivationFunctionCreateTanh(hidden) if act is None else act
        self.cfg = L.RNNConfigCreate(in_features, hidden, return_sequences, timesteps, v2, self.act)
        # mini_batch: a *CreateForTraining handle of that mini-batch size (the training calls), else an inference handle
        self.mini_batch = mini_batch
        self.h = (L.RNNCreateForTraining(self.cfg, capi.ConvTrainingConfig(mini_batch)) if mini_batch else
                  L.RNNCreateForInference(self.cfg))
        self._get_weights, self._apply, self._apply_batch = L.RNNGetWeights, L.RNNApplyInference, L.RNNApplyInferenceBatch
        self._apply_device, self._sync, self._reset = L.RNNApplyDevice, L.RNNSyncWeights, L.RNNResetState
        self._apply_device_vl, self._is_lstm = L.RNNApplyDeviceVarLen, False
        self._destroy = L.RNNDestroy
        self.acts = self.act
        self._acts_destroy = L.ActivationFunctionDestroy

    def state(self):
        H = self.cfg.base.output_feature_channels
        h = np.empty(H, np.float32)
        check(capi.load().RNNGetState(self.h, _p(h)), "RNNGetState")
        return h


def bd_reverse_device(x, kind="input", lengths=None):
    """[B,T,F] device tensor with every sequence's rows in reverse time order (bidirectional.h).  lengths (one per row):
    reverse each row's first lengths[b] steps and zero the rest (bd_reverse_*_batch_varlen_device)."""
    import torch
    L = capi.load()
    B, T, F = x.shape
    cfg = capi.RecurrentConfig(F, F, True, T)
    out = torch.empty_like(x)
    if lengths is not None:
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        assert lens.shape[0] == B, "lengths: one per row"
        fn = L.bd_reverse_input_batch_varlen_device if kind == "input" else L.bd_reverse_backward_batch_varlen_device
        check(fn(_dp(x), _dp(out), cfg, B, lens.ctypes.data_as(capi.ip)), "bd_reverse_*_varlen_device")
        return out
    fn = L.bd_reverse_input_batch_device if kind == "input" else L.bd_reverse_backward_batch_device
    check(fn(_dp(x), _dp(out), cfg, B), "bd_reverse_*_device")
    return out


def bd_merge_device(fwd, bwd, mode="concat"):
    """fwd, bwd: [B,rows,C] (or [B,C]) device tensors -> concat along features or sum."""
    import torch
    L = capi.load()
    seq = fwd.dim() == 3
    B, Cc = fwd.shape[0], fwd.shape[-1]
    rows = fwd.shape[1] if seq else 1
    cfg = capi.RecurrentConfig(Cc, Cc, seq, rows)
    if mode == "concat":
        out = torch.empty(fwd.shape[:-1] + (2 * Cc,), device=fwd.device)
        check(L.bd_merge_concat_device(_dp(fwd), _dp(bwd), _dp(out), cfg, B), "bd_merge_concat_device")
    else:
        out = torch.empty_like(fwd)
        check(L.bd_merge_sum_device(_dp(fwd), _dp(bwd), _dp(out), cfg, B), "bd_merge_sum_device")
    return out


_BD_MERGE = {"concat": 0, "sum": 1}


def _bd_args(fwd, x_shape, lengths, merge):
    base = fwd.cfg.base
    B, H, T = x_shape[0], base.output_feature_channels, base.timesteps
    W = 2 * H if merge == "concat" else H
    shape = (B, T, W) if base.return_sequences else (B, W)
    lens, lp = None, None
    if lengths is not None:
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        assert lens.shape[0] == B, "lengths: one per row"
        lp = lens.ctypes.data_as(capi.ip)
    return B, shape, _BD_MERGE.get(merge, -1), lens, lp


def bidirectional_apply_device(fwd, bwd, x, lengths=None, merge="concat", out=None):
    """``<Layer>BidirectionalApplyDevice``: a bidirectional layer of two GRU / LSTM / RNN layers of one kind (the same object may be
    passed twice) in one call.  x [B,T,in] device tensor; lengths: one per row, or None for all T; merge "concat" ([...,2H]) or "sum"."""
    kind = type(fwd).__name__
    B, shape, m, lens, lp = _bd_args(fwd, x.shape, lengths, merge)
    if out is None:
        out = x.new_empty(shape)
    fn = getattr(capi.load(), kind + "BidirectionalApplyDevice")
    check(fn(fwd.h, bwd.h, _dp(x), _dp(out), B, lp, m), kind + "BidirectionalApplyDevice")
    return out


def bidirectional_apply(fwd, bwd, x, lengths=None, merge="concat"):
    """The host-memory form (``<Layer>BidirectionalApplyInferenceBatch``): x [B,T,in] numpy array."""
    kind = type(fwd).__name__
    x = _f32(x)
    B, shape, m, lens, lp = _bd_args(fwd, x.shape, lengths, merge)
    out = np.empty(shape, np.float32)
    fn = getattr(capi.load(), kind + "BidirectionalApplyInferenceBatch")
    check(fn(fwd.h, bwd.h, _p(x), _p(out), B, lp, m), kind + "BidirectionalApplyInferenceBatch")
    return out


def bidirectional_train_forward_device(fwd, bwd, x, lengths=None, merge="concat", out=None):
    """``<Layer>BidirectionalApplyTrainingBatchDevice``: the training forward of a bidirectional layer in one call.  fwd, bwd: two
    different layers of one kind created with ``mini_batch=B``; x [B,T,in] device tensor, which must stay alive until the backward call;
    lengths: one per row, or None for all T; merge "concat" ([...,2H]) or "sum".  Rows past a length are zeros."""
    kind = type(fwd).__name__
    B, shape, m, lens, lp = _bd_args(fwd, x.shape, lengths, merge)
    if B != fwd.mini_batch:
        raise ValueError("%sBidirectionalApplyTrainingBatchDevice: x must hold the handles' mini_batch = %s rows" % (kind, fwd.mini_batch))
    if out is None:
        out = x.new_empty(shape)
    name = kind + "BidirectionalApplyTrainingBatchDevice"
    check(getattr(capi.load(), name)(fwd.h, bwd.h, _dp(x), _dp(out), lp, m), name)
    return out


def bidirectional_train_backward_device(fwd, bwd, dout, grad_fwd, grad_bwd, dX=None):
    """``<Layer>BidirectionalCalculateGradientDevice`` after bidirectional_train_forward_device on the same pair: dout in the forward
    call's output layout; grad_fwd / grad_bwd: device tensors of each direction's block W | U | b_i | b_h, ADDED to; returns dX [B,T,in]
    (written; zeros past a row's length)."""
    kind = type(fwd).__name__
    base = fwd.cfg.base
    if dX is None:
        dX = dout.new_empty((fwd.mini_batch, base.timesteps, base.input_feature_channels))
    name = kind + "BidirectionalCalculateGradientDevice"
    check(getattr(capi.load(), name)(fwd.h, bwd.h, _dp(grad_fwd), _dp(grad_bwd), _dp(dX), _dp(dout)), name)
    return dX


def _ctc_labels(labels, label_lengths, B):
    """labels as a list of per-row lists, or a padded int array [B, max_label_len] plus label_lengths -> (int32 [B, maxL], int32 [B])"""
    if label_lengths is None:
        rows = [np.asarray(r, dtype=np.int32).reshape(-1) for r in labels]
        assert len(rows) == B, "labels: one list per row"
        lens = np.array([r.shape[0] for r in rows], dtype=np.int32)
        lab = np.zeros((B, max(1, int(lens.max()) if B else 1)), np.int32)
        for b, r in enumerate(rows):
            lab[b, :r.shape[0]] = r
        return lab, lens
    lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32)).reshape(B, -1)
    return lab, _host_ints(label_lengths, B, "label_lengths")


def _ctc_lengths(input_lengths, B):
    if input_lengths is None:
        return None, None
    lens = _host_ints(input_lengths, B, "input_lengths")
    return lens, lens.ctypes.data_as(capi.ip)


def ctc_loss_device(probs, labels, label_lengths=None, input_lengths=None, blank=0, want_grad=True, loss=None, dprobs=None, workspace=None):
    """``nntk_ctc_loss_device``: probs [B,T,C] device tensor of softmax PROBABILITIES; labels: a list of per-row lists, or a padded
    int array [B, max_label_len] with label_lengths.  Returns (loss rows [B], d loss / d probs [B,T,C] or None)."""
    import torch
    B, T, Cc = probs.shape
    lab, ll = _ctc_labels(labels, label_lengths, B)
    il, ilp = _ctc_lengths(input_lengths, B)
    L = capi.load()
    need = L.nntk_ctc_workspace_floats(B, T if want_grad else 0, lab.shape[1])
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=probs.device)
    assert workspace.numel() >= need, "workspace: nntk_ctc_workspace_floats(B, T, max_label_len) floats"
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=probs.device)
    if want_grad and dprobs is None:
        dprobs = torch.empty_like(probs)
    check(L.nntk_ctc_loss_device(_dp(probs), B, T, Cc, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), lab.shape[1], blank,
                                 _dp(loss), _dp(dprobs) if want_grad else None, _dp(workspace)), "nntk_ctc_loss_device")
    return loss, (dprobs if want_grad else None)


def ctc_loss(probs, labels, label_lengths=None, input_lengths=None, blank=0, want_grad=True):
    """The host-memory form (``nntk_ctc_loss``): probs [B,T,C] numpy array."""
    probs = _f32(probs)
    B, T, Cc = probs.shape
    lab, ll = _ctc_labels(labels, label_lengths, B)
    il, ilp = _ctc_lengths(input_lengths, B)
    loss = np.empty(B, np.float32)
    g = np.empty_like(probs) if want_grad else None
    check(capi.load().nntk_ctc_loss(_p(probs), B, T, Cc, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), lab.shape[1], blank,
                                    _p(loss), _p(g) if want_grad else None), "nntk_ctc_loss")
    return loss, g


def ctc_greedy_decode_device(probs, input_lengths=None, blank=0, labels_out=None, out_lengths=None):
    """``nntk_ctc_greedy_decode_device``: best path of probs [B,T,C] -> (labels [B,T] int32, -1 behind each row's labels; lengths [B])"""
    import torch
    B, T, Cc = probs.shape
    il, ilp = _ctc_lengths(input_lengths, B)
    if labels_out is None:
        labels_out = torch.empty((B, T), dtype=torch.int32, device=probs.device)
    if out_lengths is None:
        out_lengths = torch.empty(B, dtype=torch.int32, device=probs.device)
    check(capi.load().nntk_ctc_greedy_decode_device(_dp(probs), B, T, Cc, ilp, blank, C.c_void_p(labels_out.data_ptr()),
                                                    C.c_void_p(out_lengths.data_ptr())), "nntk_ctc_greedy_decode_device")
    return labels_out, out_lengths


def ctc_greedy_decode(probs, input_lengths=None, blank=0):
    """The host-memory form (``nntk_ctc_greedy_decode``): probs [B,T,C] numpy array."""
    probs = _f32(probs)
    B, T, Cc = probs.shape
    il, ilp = _ctc_lengths(input_lengths, B)
    out, n = np.empty((B, T), np.int32), np.empty(B, np.int32)
    check(capi.load().nntk_ctc_greedy_decode(_p(probs), B, T, Cc, ilp, blank, out.ctypes.data_as(capi.ip), n.ctypes.data_as(capi.ip)),
          "nntk_ctc_greedy_decode")
    return out, n


def _ctc_beam_arrays(device, B, nbest, L, detail, given=(None, None, None)):
    """The outputs of a CTC beam search: labels [B, nbest, L] int32, lengths [B, nbest] int32, scores [B, nbest] float32 and, with
    detail, label_frames int32 and label_logps float32 [B, nbest, L].  Tensors on ``device`` -- the caller's (``given``: labels_out,
    out_lengths, scores) where it passed some -- or, device None, numpy arrays.  -> (the arrays, their addresses as the C entries
    take them: untyped for device tensors, typed for numpy arrays)"""
    shapes = [((B, nbest, L), "int32"), ((B, nbest), "int32"), ((B, nbest), "float32")]
    shapes += [((B, nbest, L), "int32"), ((B, nbest, L), "float32")] if detail else []
    if device is None:
        outs = tuple(np.empty(s, d) for s, d in shapes)
        return outs, [a.ctypes.data_as(fp if a.dtype == np.float32 else capi.ip) for a in outs]
    import torch
    outs = tuple(torch.empty(s, dtype=getattr(torch, d), device=device) if g is None else g
                 for (s, d), g in zip(shapes, tuple(given) + (None, None)))
    for a, (_, d) in zip(outs, shapes):
        assert a.is_cuda and a.is_contiguous() and a.dtype == getattr(torch, d), "outputs: contiguous device tensors, int32 / float32"
    return outs, [C.c_void_p(a.data_ptr()) for a in outs]


def _ctc_beam_decode(on_device, lm_entry, lm, probs, input_lengths, blank, beam_width, cutoff_top_n, nbest, detail,
                     given=(None, None, None), workspace=None):
    """The one-shot search in all its forms.  on_device: probs and the outputs are device tensors, else numpy arrays; lm_entry: the
    caller is one of the ``_lm`` functions, whose model ``lm`` may still be None.  The C entry is the calling function's own:
    ``nntk_ctc_beam_decode`` + ``_opt`` (NntkCtcBeamOptions) with detail, else ``_lm`` for an ``_lm`` function, + ``_device``."""
    if not on_device:
        probs = _f32(probs)
    B, T, Cc = probs.shape
    il, ilp = _ctc_lengths(input_lengths, B)
    L = capi.load()
    outs, ptrs = _ctc_beam_arrays(probs.device if on_device else None, B, max(nbest, 0), T, detail, given)
    lm_h = lm.h if lm is not None else None
    if detail:
        form, mid = "_opt", (C.byref(capi.NntkCtcBeamOptions(lm_h, *(C.cast(q, C.c_void_p) for q in ptrs[3:]))),)
    elif lm_entry:
        form, mid = "_lm", (lm_h,)
    else:
        form, mid = "", ()
    tail = ()
    if on_device:
        import torch
        ws_name = "nntk_ctc_beam_lm_workspace_floats" if lm_entry else "nntk_ctc_beam_workspace_floats"
        need = getattr(L, ws_name)(B, T, Cc, beam_width, cutoff_top_n)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.float32, device=probs.device)
        assert workspace.numel() >= need, "workspace: %s(B, T, C, beam_width, cutoff_top_n) floats" % ws_name
        tail = (_dp(workspace),)
    name = "nntk_ctc_beam_decode" + form + ("_device" if on_device else "")
    check(getattr(L, name)((_dp if on_device else _p)(probs), B, T, Cc, ilp, blank, beam_width, cutoff_top_n, nbest, *mid, *ptrs[:3],
                           *tail), name)
    return outs


def ctc_beam_decode_device(probs, input_lengths=None, blank=0, beam_width=16, cutoff_top_n=0, nbest=1, labels_out=None, out_lengths=None,
                           scores=None, workspace=None, detail=False):
    """``nntk_ctc_beam_decode_device``: prefix beam search over probs [B,T,C] -> (labels [B,nbest,T] int32, -1 behind each hypothesis'
    labels; lengths [B,nbest] int32, -1 for a slot without a hypothesis; scores [B,nbest] float32 = ln of the prefix probability).
    ``detail=True`` (``nntk_ctc_beam_decode_opt_device``): the same three and (label_frames [B,nbest,T] int32, -1 behind the labels';
    label_logps [B,nbest,T] float32, 0.0 behind them) -- INTEGRATION.md "Label timestamps and confidences"."""
    return _ctc_beam_decode(True, False, None, probs, input_lengths, blank, beam_width, cutoff_top_n, nbest, detail, (labels_out, out_lengths, scores),
                            workspace)


def ctc_beam_decode(probs, input_lengths=None, blank=0, beam_width=16, cutoff_top_n=0, nbest=1, detail=False):
    """The host-memory form (``nntk_ctc_beam_decode``, with detail ``nntk_ctc_beam_decode_opt``): probs [B,T,C] numpy array."""
    return _ctc_beam_decode(False, False, None, probs, input_lengths, blank, beam_width, cutoff_top_n, nbest, detail)


class NgramLm:
    """``nntk_ngram_lm_*``: a token-level n-gram language model as a deterministic backoff automaton, for ``ctc_beam_decode_lm_device``
    and ``CtcBeamStream(lm=...)`` (INTEGRATION.md "CTC prefix beam search", Language-model fusion) and for the transducer's
    ``RnntDecoder.beam_decode(lm=...)`` and ``RnntBeamStream(lm=...)``.  Log-probabilities are natural."""

    def __init__(self, h, n_states):
        self.h, self.n_states = h, n_states

    @classmethod
    def from_arrays(cls, n_classes, blank, arc_begin, arc_label, arc_logp, arc_next, backoff_state, backoff_logw, final_logp=None,
                    start_state=0, unk_logp=-np.inf, alpha=1.0, beta=0.0):
        ab = np.ascontiguousarray(np.asarray(arc_begin, dtype=np.int64).reshape(-1))
        assert C.sizeof(C.c_long) == 8 and ab.shape[0] >= 2, "arc_begin: n_states + 1 entries"
        ns = ab.shape[0] - 1
        ints = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
        al, an, bs = ints(arc_label), ints(arc_next), ints(backoff_state)
        ap, bw = _f32(arc_logp).reshape(-1), _f32(backoff_logw).reshape(-1)
        fl = None if final_logp is None else _f32(final_logp).reshape(-1)
        assert al.shape[0] == an.shape[0] == ap.shape[0], "arc_label, arc_logp, arc_next: one entry per arc"
        assert bs.shape[0] == bw.shape[0] == ns and (fl is None or fl.shape[0] == ns), "backoff_state, backoff_logw, final_logp: one entry per state"
        na = al.shape[0]
        assert ab.size == 0 or int(ab.max()) <= na, "arc_begin points past the arc arrays"
        h = capi.load().nntk_ngram_lm_create(int(n_classes), int(blank), ns, ab.ctypes.data_as(C.POINTER(C.c_long)),
                                             al.ctypes.data_as(capi.ip), _p(ap), an.ctypes.data_as(capi.ip), bs.ctypes.data_as(capi.ip),
                                             _p(bw), None if fl is None else _p(fl), int(start_state), float(unk_logp), float(alpha),
                                             float(beta))
        if not h:
            raise capi.NNTKError("nntk_ngram_lm_create: " + capi.last_error())
        return cls(h, ns)

    @staticmethod
    def arpa_arrays(text, classes, unk_logp=-np.inf):
        """The automaton of an ARPA file's text.  ``classes``: token -> class index.  log10 becomes ln; the states are the contexts
        that occur (as a history of some n-gram, or as the n-1 last tokens of a non-final one), shortest first; ``<s>`` is dropped
        as a label and the start state is the context (<s>) when there is one; ``</s>`` becomes final_logp, backed off.
        -> dict of from_arrays' array arguments"""
        ln10 = float(np.log(10.0))
        grams, order = {}, 0
        for line in text.splitlines():
            line = line.strip()
            if line.startswith("\\") and line.endswith("-grams:"):
                order = int(line[1:line.index("-")])
            elif line.startswith("\\") or not line or line.startswith("ngram "):
                order = 0 if line.startswith("\\") else order
            elif order:
                f = line.split()
                toks = tuple(f[1:1 + order])
                grams[toks] = (float(f[0]) * ln10, float(f[1 + order]) * ln10 if len(f) > 1 + order else 0.0)
        nmax = max((len(g) for g in grams), default=1)
        ctxs = {()}
        for g in grams:
            if "</s>" not in g[:-1]:
                ctxs.add(g[:-1])
                if len(g) < nmax and g[-1] != "</s>":
                    ctxs.add(g)
        ctxs = {c for c in ctxs if "<s>" not in c[1:]}
        closed = set()
        for c in ctxs:                                   # every suffix of a context is a context: the backoff chain
            while c not in closed:
                closed.add(c)
                c = c[1:]
        order_ctx = sorted(closed, key=lambda c: (len(c), c))
        sid = {c: i for i, c in enumerate(order_ctx)}

        def longest(c):
            while c not in sid:
                c = c[1:]
            return sid[c]
        arc_begin, arc_label, arc_logp, arc_next, bo_state, bo_logw, final = [0], [], [], [], [], [], []
        for c in order_ctx:
            arcs = sorted((classes[g[-1]], lp, g) for g, (lp, _) in grams.items()
                          if g[:-1] == c and g[-1] in classes and g[-1] not in ("<s>", "</s>"))
            for k, lp, g in arcs:
                arc_label.append(k); arc_logp.append(lp); arc_next.append(longest(g[-(nmax - 1):] if nmax > 1 else ()))
            arc_begin.append(len(arc_label))
            bo_state.append(-1 if not c else longest(c[1:]))
            bo_logw.append(grams.get(c, (0.0, 0.0))[1] if c else 0.0)
            f, cc = 0.0, c                               # </s> from this context, backed off
            while cc + ("</s>",) not in grams and cc:
                f += grams.get(cc, (0.0, 0.0))[1]
                cc = cc[1:]
            final.append(f + grams[cc + ("</s>",)][0] if cc + ("</s>",) in grams else -np.inf)
        return dict(arc_begin=arc_begin, arc_label=arc_label, arc_logp=arc_logp, arc_next=arc_next, backoff_state=bo_state,
                    backoff_logw=bo_logw, final_logp=final, start_state=sid.get(("<s>",), 0), unk_logp=unk_logp)

    @classmethod
    def from_arpa(cls, text, classes, blank, alpha=1.0, beta=0.0, unk_logp=-np.inf):
        """``classes``: token -> class index (the blank has no token).  Not a hot path: pure Python."""
        n_classes = max(list(classes.values()) + [blank]) + 1
        return cls.from_arrays(n_classes, blank, alpha=alpha, beta=beta, **cls.arpa_arrays(text, classes, unk_logp))

    def score(self, labels, with_final=False):
        """sum of ln F along labels (+ ln E of the last state): what the fused score holds beyond the acoustic one.  Host only."""
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32).reshape(-1))
        v = capi.load().nntk_ngram_lm_score(self.h, lab.ctypes.data_as(capi.ip), lab.shape[0], int(bool(with_final)))
        if v != v:
            raise capi.NNTKError("nntk_ngram_lm_score: " + capi.last_error())
        return v

    def device_bytes(self):
        return capi.load().nntk_ngram_lm_device_bytes(self.h)

    def rnnt_device_bytes(self):
        """the doubles the transducer beam search reads next to the lookup records of ``device_bytes``"""
        return capi.load().nntk_ngram_lm_rnnt_device_bytes(self.h)

    def close(self):
        if self.h:
            capi.load().nntk_ngram_lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ctc_beam_decode_lm_device(probs, lm, input_lengths=None, blank=0, beam_width=16, cutoff_top_n=0, nbest=1, labels_out=None,
                              out_lengths=None, scores=None, workspace=None, detail=False):
    """``nntk_ctc_beam_decode_lm_device``: ``ctc_beam_decode_device`` with the n-gram model ``lm`` (an NgramLm, or None) fused in;
    scores = ln(acoustic prefix probability x LM factors x end-of-sentence factor).  ``detail=True``: as in ``ctc_beam_decode_device``
    (label_logps stays the acoustic log-probability, never the model's factor)."""
    return _ctc_beam_decode(True, True, lm, probs, input_lengths, blank, beam_width, cutoff_top_n, nbest, detail,
                            (labels_out, out_lengths, scores), workspace)


def ctc_beam_decode_lm(probs, lm, input_lengths=None, blank=0, beam_width=16, cutoff_top_n=0, nbest=1, detail=False):
    """The host-memory form (``nntk_ctc_beam_decode_lm``, with detail ``nntk_ctc_beam_decode_opt``): probs [B,T,C] numpy array."""
    return _ctc_beam_decode(False, True, lm, probs, input_lengths, blank, beam_width, cutoff_top_n, nbest, detail)


class CtcBeamStream:
    """``nntk_ctc_beam_stream_*``: prefix beam search pushed chunk by chunk for ``batch`` independent streams.  After every push row
    b holds what ``ctc_beam_decode_device`` gives on the row's frames since its last reset, bit for bit (INTEGRATION.md "CTC prefix
    beam search", Streaming).  ``max_labels``: the capacity of the returned label strings (default: max_frames).  ``lm``: an NgramLm
    fused in as by ``ctc_beam_decode_lm_device``; it must outlive the stream.  ``detail=True`` (``nntk_ctc_beam_stream_create_opt``):
    the rows also carry their labels' frames (counted from the row's last reset) and log-probabilities, and ``push`` / ``push_host``
    return (labels, lengths, scores, label_frames, label_logps), the last two [B, nbest, max_labels]."""

    def __init__(self, batch, max_frames, C, blank=0, beam_width=16, cutoff_top_n=0, nbest=1, max_labels=None, lm=None, detail=False):
        self.B, self.T, self.C, self.nbest = int(batch), int(max_frames), int(C), int(nbest)
        self.max_labels = int(max_frames if max_labels is None else max_labels)
        self.lm = lm
        self.detail = bool(detail)
        if self.detail:
            form, mid = "_opt", (lm.h if lm is not None else None, 1)
        elif lm is not None:
            form, mid = "_lm", (lm.h,)
        else:
            form, mid = "", ()
        self.h = getattr(capi.load(), "nntk_ctc_beam_stream_create" + form)(self.B, self.T, self.C, blank, beam_width, cutoff_top_n, nbest,
                                                                            self.max_labels, *mid)
        if not self.h:
            raise capi.NNTKError("nntk_ctc_beam_stream_create: " + capi.last_error())

    def _final(self, final):
        if final is None:
            return None, None
        f = _host_ints(np.asarray(final).astype(np.int32), self.B, "final")
        return f, f.ctypes.data_as(capi.ip)

    def push(self, probs, n_frames, final=None, labels_out=None, out_lengths=None, scores=None):
        """probs [B, max_frames, C] device tensor, n_frames / final host ints per row (a streaming stack's out, cnt, final) ->
        (labels [B, nbest, max_labels] int32, lengths [B, nbest] int32, scores [B, nbest] float32), the rows' current n-best"""
        return self._push(True, probs, n_frames, final, (labels_out, out_lengths, scores))

    def push_host(self, probs, n_frames, final=None):
        """The host-memory form (``nntk_ctc_beam_stream_push``): probs [B, max_frames, C] numpy array."""
        return self._push(False, _f32(probs), n_frames, final)

    def _push(self, on_device, probs, n_frames, final, given=(None, None, None)):
        """both forms of a push, through ``nntk_ctc_beam_stream_push`` + ``_opt`` on a handle with detail + ``_device``"""
        assert tuple(probs.shape) == (self.B, self.T, self.C), "probs: [batch, max_frames, C]"
        nf = _host_ints(n_frames, self.B, "n_frames")
        f, fptr = self._final(final)
        outs, ptrs = _ctc_beam_arrays(probs.device if on_device else None, self.B, self.nbest, self.max_labels, self.detail, given)
        name = "nntk_ctc_beam_stream_push" + ("_opt" if self.detail else "") + ("_device" if on_device else "")
        check(getattr(capi.load(), name)(self.h, (_dp if on_device else _p)(probs), nf.ctypes.data_as(capi.ip), fptr, *ptrs), name)
        return outs

    def reset(self, rows):
        """these rows start new streams"""
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        check(capi.load().nntk_ctc_beam_stream_reset(self.h, rows.ctypes.data_as(capi.ip), rows.shape[0]), "nntk_ctc_beam_stream_reset")

    def close(self):
        if self.h:
            capi.load().nntk_ctc_beam_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ctc_greedy_decode_stream_device(probs, n_frames, prev, blank=0, labels_out=None, out_lengths=None):
    """``nntk_ctc_greedy_decode_stream_device``: the labels this chunk adds.  probs [B,T,C]; n_frames host ints per row; prev [B] int32
    device tensor, updated in place (-1 = a new stream) -> (labels [B,T] int32, -1 behind each row's labels; lengths [B])"""
    import torch
    B, T, Cc = probs.shape
    nf = _host_ints(n_frames, B, "n_frames")
    assert prev.is_cuda and prev.dtype == torch.int32 and prev.is_contiguous() and prev.numel() == B, "prev: [B] int32 device tensor"
    if labels_out is None:
        labels_out = torch.empty((B, T), dtype=torch.int32, device=probs.device)
    if out_lengths is None:
        out_lengths = torch.empty(B, dtype=torch.int32, device=probs.device)
    check(capi.load().nntk_ctc_greedy_decode_stream_device(_dp(probs), B, T, Cc, nf.ctypes.data_as(capi.ip), blank,
                                                           C.c_void_p(prev.data_ptr()), C.c_void_p(labels_out.data_ptr()),
                                                           C.c_void_p(out_lengths.data_ptr())), "nntk_ctc_greedy_decode_stream_device")
    return labels_out, out_lengths


def ctc_align_device(probs, labels, label_lengths=None, input_lengths=None, blank=0, states=None, spans=None, scores=None, workspace=None):
    """``nntk_ctc_align_device``: the best alignment of probs [B,T,C] to the labels (as for ``ctc_loss_device``) -> (states [B,T] int32,
    the extended state of every frame, -1 behind each row; spans [B,max_label_len,2] int32, each label's first frame and one past
    its last, -1 for a label the row does not have; scores [B] float32 = ln of the path's probability, -inf where there is no path)"""
    import torch
    B, T, Cc = probs.shape
    lab, ll = _ctc_labels(labels, label_lengths, B)
    il, ilp = _ctc_lengths(input_lengths, B)
    L = capi.load()
    need = L.nntk_ctc_align_workspace_floats(B, T, lab.shape[1])
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=probs.device)
    assert workspace.numel() >= need, "workspace: nntk_ctc_align_workspace_floats(B, T, max_label_len) floats"
    if states is None:
        states = torch.empty((B, T), dtype=torch.int32, device=probs.device)
    if spans is None:
        spans = torch.empty((B, lab.shape[1], 2), dtype=torch.int32, device=probs.device)
    if scores is None:
        scores = torch.empty(B, dtype=torch.float32, device=probs.device)
    check(L.nntk_ctc_align_device(_dp(probs), B, T, Cc, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), lab.shape[1], blank,
                                  C.c_void_p(states.data_ptr()), C.c_void_p(spans.data_ptr()), _dp(scores), _dp(workspace)),
          "nntk_ctc_align_device")
    return states, spans, scores


def ctc_align(probs, labels, label_lengths=None, input_lengths=None, blank=0):
    """The host-memory form (``nntk_ctc_align``): probs [B,T,C] numpy array."""
    probs = _f32(probs)
    B, T, Cc = probs.shape
    lab, ll = _ctc_labels(labels, label_lengths, B)
    il, ilp = _ctc_lengths(input_lengths, B)
    st, sp, sc = np.empty((B, T), np.int32), np.empty((B, lab.shape[1], 2), np.int32), np.empty(B, np.float32)
    check(capi.load().nntk_ctc_align(_p(probs), B, T, Cc, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), lab.shape[1], blank,
                                     st.ctypes.data_as(capi.ip), sp.ctypes.data_as(capi.ip), _p(sc)), "nntk_ctc_align")
    return st, sp, sc


def _edit_refs(refs, ref_lengths, B):
    """references as the labels of ``ctc_loss_device`` (a list of per-row lists, or a padded int array with ref_lengths) ->
    (int32 [B, max_ref_len], int32 [B])"""
    lab, ll = _ctc_labels(refs, ref_lengths, B)
    return np.ascontiguousarray(lab), ll


def edit_distance_device(hyp, hyp_lengths, refs, ref_lengths=None, sep=-1, counts=None, ref_units=None, workspace=None):
    """``nntk_edit_distance_device``: hyp [B,n_hyp,L] int32 device tensor with hyp_lengths [B,n_hyp], as the beam searches leave them
    (or [B,L] with [B], the greedy decoders: n_hyp = 1); refs as the labels of the loss calls, HOST memory.  sep < 0 compares tokens,
    sep >= 0 the words between separators.  Returns (counts [B,n_hyp,4] int32 = {distance, substitutions, deletions, insertions},
    -1 for a slot without a hypothesis; ref_units [B] int32, the references' tokens or words)."""
    import torch
    if hyp.dim() == 2:
        hyp = hyp.unsqueeze(1)
    B, n_hyp, Lh = hyp.shape
    assert hyp_lengths.numel() == B * n_hyp, "hyp_lengths: one per hypothesis"
    ref, rl = _edit_refs(refs, ref_lengths, B)
    L = capi.load()
    need = L.nntk_edit_distance_workspace_floats(B, n_hyp, Lh, ref.shape[1])
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=hyp.device)
    assert workspace.numel() >= need, "workspace: nntk_edit_distance_workspace_floats(B, n_hyp, max_hyp_len, max_ref_len) floats"
    if counts is None:
        counts = torch.empty((B, n_hyp, 4), dtype=torch.int32, device=hyp.device)
    if ref_units is None:
        ref_units = torch.empty(B, dtype=torch.int32, device=hyp.device)
    check(L.nntk_edit_distance_device(_ip(hyp), _ip(hyp_lengths), B, n_hyp, Lh, ref.ctypes.data_as(capi.ip), rl.ctypes.data_as(capi.ip),
                                      ref.shape[1], sep, _ip(counts), _ip(ref_units), _dp(workspace)), "nntk_edit_distance_device")
    return counts, ref_units


def edit_distance(hyp, hyp_lengths, refs, ref_lengths=None, sep=-1):
    """The host-memory form (``nntk_edit_distance``): hyp [B,n_hyp,L] (or [B,L]) and hyp_lengths numpy int arrays."""
    hyp = np.ascontiguousarray(np.asarray(hyp, dtype=np.int32))
    if hyp.ndim == 2:
        hyp = hyp[:, None, :]
    B, n_hyp, Lh = hyp.shape
    hl = np.ascontiguousarray(np.asarray(hyp_lengths, dtype=np.int32).reshape(-1))
    assert hl.shape[0] == B * n_hyp, "hyp_lengths: one per hypothesis"
    ref, rl = _edit_refs(refs, ref_lengths, B)
    counts, units = np.empty((B, n_hyp, 4), np.int32), np.empty(B, np.int32)
    check(capi.load().nntk_edit_distance(hyp.ctypes.data_as(capi.ip), hl.ctypes.data_as(capi.ip), B, n_hyp, Lh, ref.ctypes.data_as(capi.ip),
                                         rl.ctypes.data_as(capi.ip), ref.shape[1], sep, counts.ctypes.data_as(capi.ip),
                                         units.ctypes.data_as(capi.ip)), "nntk_edit_distance")
    return counts, units


def error_rate(counts, ref_units):
    """The corpus error rate of the first hypothesis of every row: sum of counts[b, 0, 0] over sum of ref_units[b] (the token error
    rate in unit mode, the word error rate in word mode).  counts / ref_units: what ``edit_distance`` or ``edit_distance_device``
    returned (device tensors are downloaded).  A row whose slot 0 holds no hypothesis counts as all deletions."""
    c = counts.cpu().numpy() if hasattr(counts, "cpu") else np.asarray(counts)
    u = ref_units.cpu().numpy() if hasattr(ref_units, "cpu") else np.asarray(ref_units)
    d = c.reshape(u.shape[0], -1, 4)[:, 0, 0].astype(np.int64)
    d = np.where(d < 0, u.astype(np.int64), d)
    total = int(u.astype(np.int64).sum())
    return float(d.sum()) / total if total else float("nan")


def mwer_device(logp, counts, risk=None, dlogp=None):
    """``nntk_mwer_device``: logp [B,n_hyp] float32 device tensor, the hypotheses' log-probabilities; counts: the [B,n_hyp,4] int32
    tensor of ``edit_distance_device`` (its distance column is read in place) or a [B,n_hyp] int32 tensor of error counts; a negative
    count marks a slot without a hypothesis.  Returns (risk [B], d risk / d logp [B,n_hyp])."""
    import torch
    B, n_hyp = logp.shape
    stride = 4 if counts.dim() == 3 else 1
    assert counts.numel() == B * n_hyp * stride, "counts: [B, n_hyp, 4] or [B, n_hyp]"
    if risk is None:
        risk = torch.empty(B, dtype=torch.float32, device=logp.device)
    if dlogp is None:
        dlogp = torch.empty_like(logp)
    check(capi.load().nntk_mwer_device(_dp(logp), _ip(counts), stride, B, n_hyp, _dp(risk), _dp(dlogp)), "nntk_mwer_device")
    return risk, dlogp


def row_scale_device(x, scale, out=None):
    """``nntk_row_scale_device``: x [rows, ...] float32 device tensor, scale [rows] -> out[r] = x[r] * scale[r] (``out`` may be ``x``);
    a scale of exactly 0 gives zeros whatever the row holds."""
    import torch
    rows = scale.numel()
    assert rows > 0 and x.shape[0] == rows or x.numel() == 0, "scale: one per row of x"
    if out is None:
        out = torch.empty_like(x)
    check(capi.load().nntk_row_scale_device(_dp(x), _dp(scale), rows, x.numel() // max(rows, 1), _dp(out)), "nntk_row_scale_device")
    return out


RNNT_ACTIVATIONS = {ACT_IDENTITY: 0, ACT_TANH: 1, ACT_RELU: 2}


def _rnnt_labels(labels, label_lengths, B, maxL):
    """labels as for ``ctc_loss_device``, padded to the lattice's max_label_len = U1 - 1 -> (int32 [B, maxL], int32 [B])"""
    if label_lengths is None:
        rows = [np.asarray(r, dtype=np.int32).reshape(-1) for r in labels]
        assert len(rows) == B, "labels: one list per row"
        assert all(r.shape[0] <= maxL for r in rows), "labels: at most logits.shape[2] - 1 per row"
        lab = np.zeros((B, maxL), np.int32)
        for b, r in enumerate(rows):
            lab[b, :r.shape[0]] = r
        return lab, np.array([r.shape[0] for r in rows], dtype=np.int32)
    lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32)).reshape(B, maxL)
    return lab, _host_ints(label_lengths, B, "label_lengths")


def _rnnt_workspace(workspace, dev, size_fn, *args):
    """the workspace of a device call: at least ``size_fn(*args)`` floats (a size function of the C API, by name), made if not given"""
    import torch
    need = getattr(capi.load(), size_fn)(*args)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=dev)
    assert workspace.numel() >= need, "workspace: %s%s floats" % (size_fn, args)
    return workspace


def _rnnt_fused_dims(enc, pred, out_block):
    """enc [B,T,J], pred [B,U1,J] and the Dense block W [J,V] | b [V] (torch or numpy) -> (B, T, U1, J, V)"""
    B, T, J = enc.shape
    U1 = pred.shape[1]
    n = int(np.prod(out_block.shape))
    assert tuple(pred.shape) == (B, U1, J), "pred: [B, U1, J] with enc's B and J"
    assert n % (J + 1) == 0, "out_block: W [J, V] | b [V]"
    return B, T, U1, J, n // (J + 1)


def rnnt_loss_device(logits, labels, label_lengths=None, input_lengths=None, blank=0, want_grad=True, loss=None, dlogits=None, workspace=None):
    """``nntk_rnnt_loss_device``: logits [B,T,U1,V] device tensor of UNNORMALISED scores (U1 = max_label_len + 1); labels: a list of
    per-row lists, or a padded int array [B, U1 - 1] with label_lengths.  Returns (loss rows [B], d loss / d logits [B,T,U1,V] or None)."""
    import torch
    B, T, U1, V = logits.shape
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    workspace = _rnnt_workspace(workspace, logits.device, "nntk_rnnt_workspace_floats", B, T, U1 - 1, int(want_grad))
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    if want_grad and dlogits is None:
        dlogits = torch.empty_like(logits)
    check(capi.load().nntk_rnnt_loss_device(_dp(logits), B, T, V, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank,
                                            _dp(loss), _dp(dlogits) if want_grad else None, _dp(workspace)), "nntk_rnnt_loss_device")
    return loss, (dlogits if want_grad else None)


def rnnt_loss(logits, labels, label_lengths=None, input_lengths=None, blank=0, want_grad=True):
    """The host-memory form (``nntk_rnnt_loss``): logits [B,T,U1,V] numpy array."""
    logits = _f32(logits)
    B, T, U1, V = logits.shape
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    loss = np.empty(B, np.float32)
    g = np.empty_like(logits) if want_grad else None
    check(capi.load().nntk_rnnt_loss(_p(logits), B, T, V, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank,
                                     _p(loss), _p(g) if want_grad else None), "nntk_rnnt_loss")
    return loss, g


def rnnt_joint_device(enc, pred, activation=ACT_TANH, out=None):
    """``nntk_rnnt_joint_device``: enc [B,T,J], pred [B,U1,J] device tensors -> out [B,T,U1,J] = act(enc[b,t] + pred[b,u])"""
    B, T, J = enc.shape
    U1 = pred.shape[1]
    assert tuple(pred.shape) == (B, U1, J), "pred: [B, U1, J] with enc's B and J"
    if out is None:
        out = enc.new_empty((B, T, U1, J))
    assert tuple(out.shape) == (B, T, U1, J)
    check(capi.load().nntk_rnnt_joint_device(_dp(enc), _dp(pred), B, T, U1, J, RNNT_ACTIVATIONS[activation], _dp(out)),
          "nntk_rnnt_joint_device")
    return out


def rnnt_joint_backward_device(out, dout, activation=ACT_TANH, denc=None, dpred=None):
    """``nntk_rnnt_joint_backward_device``: the joiner's forward output and the gradient arriving at it, both [B,T,U1,J] ->
    (d enc [B,T,J], d pred [B,U1,J]), both overwritten"""
    B, T, U1, J = dout.shape
    assert tuple(out.shape) == (B, T, U1, J)
    if denc is None:
        denc = dout.new_empty((B, T, J))
    if dpred is None:
        dpred = dout.new_empty((B, U1, J))
    assert tuple(denc.shape) == (B, T, J) and tuple(dpred.shape) == (B, U1, J)
    check(capi.load().nntk_rnnt_joint_backward_device(_dp(out), _dp(dout), B, T, U1, J, RNNT_ACTIVATIONS[activation], _dp(denc), _dp(dpred)),
          "nntk_rnnt_joint_backward_device")
    return denc, dpred


def rnnt_fused_loss_device(enc, pred, out_block, labels, label_lengths=None, input_lengths=None, blank=0, activation=ACT_TANH, want_grad=True,
                           loss=None, denc=None, dpred=None, dout=None, workspace=None):
    """``nntk_rnnt_fused_loss_device``: enc [B,T,J], pred [B,U1,J] and the Dense block W [J,V] | b [V] (J V + V floats) as device tensors;
    labels as for ``rnnt_loss_device``.  Returns (loss rows [B], d enc, d pred, d out_block), the gradients of the plain sum of the loss
    rows (None without want_grad).  The [B,T,U1,V] logits are never stored."""
    import torch
    B, T, U1, J, V = _rnnt_fused_dims(enc, pred, out_block)
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    workspace = _rnnt_workspace(workspace, enc.device, "nntk_rnnt_fused_workspace_floats", B, T, U1 - 1, J, V, int(want_grad))
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=enc.device)
    if want_grad:
        denc = torch.empty_like(enc) if denc is None else denc
        dpred = torch.empty_like(pred) if dpred is None else dpred
        dout = torch.empty_like(out_block) if dout is None else dout
    check(capi.load().nntk_rnnt_fused_loss_device(_dp(enc), _dp(pred), _dp(out_block), B, T, J, V, RNNT_ACTIVATIONS[activation], ilp,
                                                  lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank, _dp(loss),
                                                  _dp(denc) if want_grad else None, _dp(dpred) if want_grad else None,
                                                  _dp(dout) if want_grad else None, _dp(workspace)), "nntk_rnnt_fused_loss_device")
    return (loss, denc, dpred, dout) if want_grad else (loss, None, None, None)


def rnnt_fused_loss(enc, pred, out_block, labels, label_lengths=None, input_lengths=None, blank=0, activation=ACT_TANH, want_grad=True):
    """The host-memory form (``nntk_rnnt_fused_loss``) on numpy arrays."""
    enc, pred, out_block = _f32(enc), _f32(pred), _f32(out_block)
    B, T, U1, J, V = _rnnt_fused_dims(enc, pred, out_block)
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    loss = np.empty(B, np.float32)
    g = (np.empty_like(enc), np.empty_like(pred), np.empty_like(out_block)) if want_grad else (None, None, None)
    check(capi.load().nntk_rnnt_fused_loss(_p(enc), _p(pred), _p(out_block), B, T, J, V, RNNT_ACTIVATIONS[activation], ilp,
                                           lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank, _p(loss),
                                           *[_p(a) if want_grad else None for a in g]), "nntk_rnnt_fused_loss")
    return (loss,) + g


def _ip(t):
    """device pointer of a contiguous int32 torch tensor"""
    import torch
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int32
    return C.c_void_p(t.data_ptr())


def rnnt_simple_loss_device(am, lm, labels, label_lengths=None, input_lengths=None, blank=0, want_grad=True, want_occ=True, loss=None,
                            dam=None, dlm=None, occ=None, workspace=None):
    """``nntk_rnnt_simple_loss_device``: am [B,T,V], lm [B,U1,V] device tensors, score(t, u, v) = am[b,t,v] + lm[b,u,v], never stored.
    Returns (loss rows [B], d am, d lm, occupancy [B,T,U1]); the gradients / the occupancy are None where not asked."""
    import torch
    B, T, V = am.shape
    U1 = lm.shape[1]
    assert tuple(lm.shape) == (B, U1, V), "lm: [B, U1, V] with am's B and V"
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    workspace = _rnnt_workspace(workspace, am.device, "nntk_rnnt_simple_workspace_floats", B, T, U1 - 1, int(want_grad or want_occ))
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=am.device)
    if want_grad:
        dam = torch.empty_like(am) if dam is None else dam
        dlm = torch.empty_like(lm) if dlm is None else dlm
    if want_occ and occ is None:
        occ = torch.empty((B, T, U1), dtype=torch.float32, device=am.device)
    check(capi.load().nntk_rnnt_simple_loss_device(_dp(am), _dp(lm), B, T, V, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip),
                                                   U1 - 1, blank, _dp(loss), _dp(dam) if want_grad else None,
                                                   _dp(dlm) if want_grad else None, _dp(occ) if want_occ else None, _dp(workspace)),
          "nntk_rnnt_simple_loss_device")
    return loss, (dam if want_grad else None), (dlm if want_grad else None), (occ if want_occ else None)


def rnnt_simple_loss(am, lm, labels, label_lengths=None, input_lengths=None, blank=0, want_grad=True, want_occ=True):
    """The host-memory form (``nntk_rnnt_simple_loss``) on numpy arrays."""
    am, lm = _f32(am), _f32(lm)
    B, T, V = am.shape
    U1 = lm.shape[1]
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    loss = np.empty(B, np.float32)
    dam, dlm = (np.empty_like(am), np.empty_like(lm)) if want_grad else (None, None)
    occ = np.empty((B, T, U1), np.float32) if want_occ else None
    check(capi.load().nntk_rnnt_simple_loss(_p(am), _p(lm), B, T, V, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank,
                                            _p(loss), *[None if a is None else _p(a) for a in (dam, dlm, occ)]), "nntk_rnnt_simple_loss")
    return loss, dam, dlm, occ


def rnnt_prune_ranges_device(occ, label_lengths, S, input_lengths=None, ranges=None, workspace=None):
    """``nntk_rnnt_prune_ranges_device``: the occupancy [B,T,U1] of ``rnnt_simple_loss_device`` -> ranges [B,T] int32 on the device: per
    frame the first of the S label positions the banded joiner and the banded loss keep"""
    import torch
    B, T, U1 = occ.shape
    ll = _host_ints(label_lengths, B, "label_lengths")
    il, ilp = _ctc_lengths(input_lengths, B)
    workspace = _rnnt_workspace(workspace, occ.device, "nntk_rnnt_prune_workspace_floats", B)
    if ranges is None:
        ranges = torch.empty((B, T), dtype=torch.int32, device=occ.device)
    check(capi.load().nntk_rnnt_prune_ranges_device(_dp(occ), B, T, ilp, ll.ctypes.data_as(capi.ip), U1 - 1, S, _ip(ranges), _dp(workspace)),
          "nntk_rnnt_prune_ranges_device")
    return ranges


def rnnt_prune_ranges(occ, label_lengths, S, input_lengths=None):
    """The host-memory form (``nntk_rnnt_prune_ranges``): occ [B,T,U1] numpy array -> ranges [B,T] int32."""
    occ = _f32(occ)
    B, T, U1 = occ.shape
    ll = _host_ints(label_lengths, B, "label_lengths")
    il, ilp = _ctc_lengths(input_lengths, B)
    ranges = np.empty((B, T), np.int32)
    check(capi.load().nntk_rnnt_prune_ranges(_p(occ), B, T, ilp, ll.ctypes.data_as(capi.ip), U1 - 1, S, ranges.ctypes.data_as(capi.ip)),
          "nntk_rnnt_prune_ranges")
    return ranges


def rnnt_pruned_joint_device(enc, pred, ranges, S, activation=ACT_TANH, out=None):
    """``nntk_rnnt_pruned_joint_device``: enc [B,T,J], pred [B,U1,J], ranges [B,T] int32 -> out [B,T,S,J] = act(enc[b,t] + pred[b,r[b,t]+s])"""
    B, T, J = enc.shape
    U1 = pred.shape[1]
    assert tuple(pred.shape) == (B, U1, J), "pred: [B, U1, J] with enc's B and J"
    assert tuple(ranges.shape) == (B, T)
    if out is None:
        out = enc.new_empty((B, T, S, J))
    assert tuple(out.shape) == (B, T, S, J)
    check(capi.load().nntk_rnnt_pruned_joint_device(_dp(enc), _dp(pred), _ip(ranges), B, T, U1, S, J, RNNT_ACTIVATIONS[activation], _dp(out)),
          "nntk_rnnt_pruned_joint_device")
    return out


def rnnt_pruned_joint_backward_device(out, dout, ranges, U1, activation=ACT_TANH, denc=None, dpred=None):
    """``nntk_rnnt_pruned_joint_backward_device``: the banded joiner's forward output and the gradient arriving at it, both [B,T,S,J] ->
    (d enc [B,T,J], d pred [B,U1,J]), both overwritten"""
    B, T, S, J = dout.shape
    assert tuple(out.shape) == (B, T, S, J) and tuple(ranges.shape) == (B, T)
    if denc is None:
        denc = dout.new_empty((B, T, J))
    if dpred is None:
        dpred = dout.new_empty((B, U1, J))
    assert tuple(denc.shape) == (B, T, J) and tuple(dpred.shape) == (B, U1, J)
    check(capi.load().nntk_rnnt_pruned_joint_backward_device(_dp(out), _dp(dout), _ip(ranges), B, T, U1, S, J, RNNT_ACTIVATIONS[activation],
                                                             _dp(denc), _dp(dpred)), "nntk_rnnt_pruned_joint_backward_device")
    return denc, dpred


def rnnt_pruned_loss_device(logits, ranges, labels, max_label_len, label_lengths=None, input_lengths=None, blank=0, want_grad=True, loss=None,
                            dlogits=None, workspace=None):
    """``nntk_rnnt_pruned_loss_device``: logits [B,T,S,V] device tensor of UNNORMALISED scores on the band ranges [B,T] (int32) of a
    lattice with U1 = max_label_len + 1.  Returns (loss rows [B], d loss / d logits [B,T,S,V] or None)."""
    import torch
    B, T, S, V = logits.shape
    assert tuple(ranges.shape) == (B, T)
    lab, ll = _rnnt_labels(labels, label_lengths, B, max_label_len)
    il, ilp = _ctc_lengths(input_lengths, B)
    workspace = _rnnt_workspace(workspace, logits.device, "nntk_rnnt_pruned_workspace_floats", B, T, max_label_len, int(want_grad))
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    if want_grad and dlogits is None:
        dlogits = torch.empty_like(logits)
    check(capi.load().nntk_rnnt_pruned_loss_device(_dp(logits), _ip(ranges), B, T, S, V, ilp, lab.ctypes.data_as(capi.ip),
                                                   ll.ctypes.data_as(capi.ip), max_label_len, blank, _dp(loss),
                                                   _dp(dlogits) if want_grad else None, _dp(workspace)), "nntk_rnnt_pruned_loss_device")
    return loss, (dlogits if want_grad else None)


def rnnt_pruned_loss(logits, ranges, labels, max_label_len, label_lengths=None, input_lengths=None, blank=0, want_grad=True):
    """The host-memory form (``nntk_rnnt_pruned_loss``): logits [B,T,S,V] and ranges [B,T] numpy arrays."""
    logits = _f32(logits)
    B, T, S, V = logits.shape
    ranges = np.ascontiguousarray(ranges, np.int32).reshape(B, T)
    lab, ll = _rnnt_labels(labels, label_lengths, B, max_label_len)
    il, ilp = _ctc_lengths(input_lengths, B)
    loss = np.empty(B, np.float32)
    g = np.empty_like(logits) if want_grad else None
    check(capi.load().nntk_rnnt_pruned_loss(_p(logits), ranges.ctypes.data_as(capi.ip), B, T, S, V, ilp, lab.ctypes.data_as(capi.ip),
                                            ll.ctypes.data_as(capi.ip), max_label_len, blank, _p(loss), _p(g) if want_grad else None),
          "nntk_rnnt_pruned_loss")
    return loss, g


def _rnnt_align_device(entry, size_fn, head, dev, dims, size_args, labels, label_lengths, input_lengths, blank, given, workspace):
    """Both device forms of the alignment: the C entry by name, its argument head (the score source: the tensors, then B, T and the
    widths as the entry takes them), dims = (B, T, U1), the workspace size function by name with its arguments, the five outputs as
    given (None: made here)"""
    import torch
    B, T, U1 = dims
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    workspace = _rnnt_workspace(workspace, dev, size_fn, *size_args)
    shapes = (((B, U1 - 1), torch.int32), ((B, T), torch.int32), ((B, U1 - 1), torch.float32), ((B, T), torch.float32), ((B,), torch.float32))
    outs = [torch.empty(s, dtype=d, device=dev) if g is None else g for (s, d), g in zip(shapes, given)]
    for o, (s, d) in zip(outs, shapes):
        assert tuple(o.shape) == s and o.dtype == d and o.is_contiguous(), "alignment outputs: %s %s" % (s, d)
    check(getattr(capi.load(), entry)(*head, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank,
                                      *[C.c_void_p(o.data_ptr()) for o in outs], _dp(workspace)), entry)
    return tuple(outs)


def _rnnt_align_host(entry, head, dims, labels, label_lengths, input_lengths, blank):
    """Both host forms of the alignment, as ``_rnnt_align_device``"""
    B, T, U1 = dims
    lab, ll = _rnnt_labels(labels, label_lengths, B, U1 - 1)
    il, ilp = _ctc_lengths(input_lengths, B)
    lf, fl = np.empty((B, U1 - 1), np.int32), np.empty((B, T), np.int32)
    lp, fp, sc = np.empty((B, U1 - 1), np.float32), np.empty((B, T), np.float32), np.empty(B, np.float32)
    check(getattr(capi.load(), entry)(*head, ilp, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), U1 - 1, blank,
                                      lf.ctypes.data_as(capi.ip), fl.ctypes.data_as(capi.ip), _p(lp), _p(fp), _p(sc)), entry)
    return lf, fl, lp, fp, sc


def rnnt_align_device(logits, labels, label_lengths=None, input_lengths=None, blank=0, label_frames=None, frame_labels=None,
                      label_logp=None, frame_logp=None, scores=None, workspace=None):
    """``nntk_rnnt_align_device``: the most probable path of logits [B,T,U1,V] (as for ``rnnt_loss_device``) through each row's labels ->
    (label_frames [B,U1-1] int32, the frame each label is emitted in, -1 behind the row's labels; frame_labels [B,T] int32, the number of
    labels emitted when each frame is left, -1 behind the row's frames; label_logp [B,U1-1] and frame_logp [B,T] float32, ln of those
    label and blank emissions, 0 in the padding; scores [B] float32 = ln of the path's probability, -inf where there is no path)"""
    B, T, U1, V = logits.shape
    return _rnnt_align_device("nntk_rnnt_align_device", "nntk_rnnt_align_workspace_floats", (_dp(logits), B, T, V), logits.device,
                              (B, T, U1), (B, T, U1 - 1), labels, label_lengths, input_lengths, blank,
                              (label_frames, frame_labels, label_logp, frame_logp, scores), workspace)


def rnnt_align(logits, labels, label_lengths=None, input_lengths=None, blank=0):
    """The host-memory form (``nntk_rnnt_align``): logits [B,T,U1,V] numpy array."""
    logits = _f32(logits)
    B, T, U1, V = logits.shape
    return _rnnt_align_host("nntk_rnnt_align", (_p(logits), B, T, V), (B, T, U1), labels, label_lengths, input_lengths, blank)


def rnnt_fused_align_device(enc, pred, out_block, labels, label_lengths=None, input_lengths=None, blank=0, activation=ACT_TANH,
                            label_frames=None, frame_labels=None, label_logp=None, frame_logp=None, scores=None, workspace=None):
    """``nntk_rnnt_fused_align_device``: the alignment of ``rnnt_align_device`` from enc [B,T,J], pred [B,U1,J] and the Dense block
    W [J,V] | b [V], as ``rnnt_fused_loss_device`` takes them; the [B,T,U1,V] logits are never stored."""
    B, T, U1, J, V = _rnnt_fused_dims(enc, pred, out_block)
    return _rnnt_align_device("nntk_rnnt_fused_align_device", "nntk_rnnt_fused_align_workspace_floats",
                              (_dp(enc), _dp(pred), _dp(out_block), B, T, J, V, RNNT_ACTIVATIONS[activation]), enc.device, (B, T, U1), (B, T, U1 - 1, J, V), labels, label_lengths, input_lengths, blank,
                              (label_frames, frame_labels, label_logp, frame_logp, scores), workspace)


def rnnt_fused_align(enc, pred, out_block, labels, label_lengths=None, input_lengths=None, blank=0, activation=ACT_TANH):
    """The host-memory form (``nntk_rnnt_fused_align``) on numpy arrays."""
    enc, pred, out_block = _f32(enc), _f32(pred), _f32(out_block)
    B, T, U1, J, V = _rnnt_fused_dims(enc, pred, out_block)
    return _rnnt_align_host("nntk_rnnt_fused_align", (_p(enc), _p(pred), _p(out_block), B, T, J, V, RNNT_ACTIVATIONS[activation]),
                            (B, T, U1), labels, label_lengths, input_lengths, blank)


def _ipv(t):
    """device pointer of a contiguous int32 torch tensor"""
    import torch
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int32
    return C.c_void_p(t.data_ptr())


def _n_frames_ptr(n_frames, B):
    """n_frames as the decode entries take it: a host int pointer (it keeps the array alive), None for None"""
    return None if n_frames is None else _host_ints(n_frames, B, "n_frames").ctypes.data_as(capi.ip)


def _rnnt_beam_entry(name, lm, opt, head, lm_args, opt_args, tail=()):
    """The one place that picks among the three C forms of a transducer beam entry -- plain, ``_lm``, ``_opt`` -- for the workspace
    size, the state, and the device and host calls.  name has ``{}`` where the forms' names differ; opt: the call takes the ``_opt``
    form (detail or length_norm; for the state, detail), else a model alone takes the ``_lm`` form.  -> (result, the entry's name)"""
    form, mid = ("_opt", opt_args) if opt else ("", ()) if lm is None else ("_lm", lm_args)
    name = name.format(form)
    return getattr(capi.load(), name)(*head, *mid, *tail), name


def _rnnt_beam_options(lm, length_norm, frames, logps):
    """NntkRnntBeamOptions by reference; frames, logps: addresses or None"""
    return C.byref(capi.NntkRnntBeamOptions(lm.h if lm is not None else None, int(bool(length_norm)), frames, logps))


def _rnnt_state_reset(entry, h, rows):
    """these rows (None: every row) of a greedy or beam stream start anew"""
    rows = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    check(getattr(capi.load(), entry)(h, *((None, 0) if rows is None else (rows.ctypes.data_as(capi.ip), rows.shape[0]))), entry)


class RnntDecoder:
    """``nntk_rnnt_decoder_*``: greedy transducer decoding with the prediction network inside the search (INTEGRATION.md
    "RNN-Transducer: greedy decoding").  Device tensors in the library's layouts: embed [V, E]; lstm_block, the flat ``LSTMGetWeights``
    block W [E,4H] | U [H,4H] | b_i | b_h; pred_proj, the flat Dense block W [H,J] | b [J], or None (identity, H == J); out, the flat
    Dense block W [J,V] | b [V].  The decoder keeps its own copy: the tensors may be freed or updated afterwards (``load_weights``)."""

    def __init__(self, embed, lstm_block, pred_proj, out, blank=0, joint_activation=ACT_TANH, max_symbols_per_frame=10):
        V, E = embed.shape
        H = self._hidden(lstm_block.numel(), E)
        J = H if pred_proj is None else pred_proj.numel() // (H + 1)
        assert pred_proj is None or pred_proj.numel() == (H + 1) * J, "pred_proj: the flat block W [H,J] | b [J]"
        assert out.numel() == (J + 1) * V, "out: the flat block W [J,V] | b [V]"
        self.V, self.E, self.H, self.J, self.max_symbols = int(V), int(E), int(H), int(J), int(max_symbols_per_frame)
        cfg = capi.NntkRnntDecoderConfig(self.V, int(blank), self.E, self.H, self.J, RNNT_ACTIVATIONS[joint_activation], self.max_symbols)
        self.h = capi.load().nntk_rnnt_decoder_create(cfg, _dp(embed), _dp(lstm_block), _dp(pred_proj) if pred_proj is not None else None,
                                                      _dp(out))
        if not self.h:
            raise capi.NNTKError("nntk_rnnt_decoder_create: " + capi.last_error())

    @staticmethod
    def _hidden(n, E):
        """H from the block's size n = 4H (E + H + 2)"""
        H = int(round((-(E + 2) + ((E + 2) ** 2 + n) ** 0.5) / 2))
        assert H >= 1 and 4 * H * (E + H + 2) == n, "lstm_block: the flat block W [E,4H] | U [H,4H] | b_i [4H] | b_h [4H]"
        return H

    def load_weights(self, embed, lstm_block, pred_proj, out):
        """``nntk_rnnt_decoder_load_weights_device``: the same four blocks, e.g. after an optimizer step"""
        check(capi.load().nntk_rnnt_decoder_load_weights_device(self.h, _dp(embed), _dp(lstm_block),
                                                                _dp(pred_proj) if pred_proj is not None else None, _dp(out)),
              "nntk_rnnt_decoder_load_weights_device")

    def _outputs(self, device, B, max_labels):
        import torch
        return (torch.empty((B, max_labels), dtype=torch.int32, device=device), torch.empty((B, max_labels), dtype=torch.int32, device=device),
                torch.empty(B, dtype=torch.int32, device=device), torch.empty(B, dtype=torch.float32, device=device))

    def _decode(self, state, enc, n_frames, max_labels, outs):
        B, T, J = enc.shape
        assert J == self.J, "enc: [B, T, J]"
        labels, frames, lengths, scores = outs
        check(capi.load().nntk_rnnt_greedy_decode_device(self.h, state, _dp(enc), B, T, _n_frames_ptr(n_frames, B), int(max_labels),
                                                         _ipv(labels), _ipv(frames), _ipv(lengths), _dp(scores)),
              "nntk_rnnt_greedy_decode_device")
        return outs

    def decode(self, enc, n_frames=None, max_labels=None):
        """enc [B, T, J] device tensor, n_frames host ints per row (None: T) -> (labels [B, max_labels] int32, -1 behind each row's
        labels; label_frames, the same shape; lengths [B] int32; scores [B] float32).  max_labels defaults to
        max_symbols_per_frame * T, which never truncates."""
        B, T, _ = enc.shape
        if max_labels is None:
            max_labels = max(1, self.max_symbols * T)
        return self._decode(None, enc, n_frames, max_labels, self._outputs(enc.device, B, max_labels))

    def _beam_outputs(self, device, B, nbest, max_labels):
        import torch
        return (torch.empty((B, nbest, max_labels), dtype=torch.int32, device=device),
                torch.empty((B, nbest), dtype=torch.int32, device=device), torch.empty((B, nbest), dtype=torch.float32, device=device))

    def _beam_detail_outputs(self, device, B, nbest, max_labels):
        import torch
        return (torch.empty((B, nbest, max_labels), dtype=torch.int32, device=device),
                torch.empty((B, nbest, max_labels), dtype=torch.float32, device=device))

    def _beam_workspace(self, device, B, beam_width, max_labels, lm=None, detail=False, length_norm=False):
        import torch
        given = 4 if detail else None                               # the size depends on whether the pointers are set, not on where they point
        need, _ = _rnnt_beam_entry("nntk_rnnt_beam{}_workspace_floats", lm, detail or length_norm, (self.h, B, int(beam_width), int(max_labels)),
                                   (), (_rnnt_beam_options(lm, length_norm, given, given),))
        return torch.empty(max(int(need), 4), dtype=torch.float32, device=device)

    def _beam(self, state, enc, n_frames, beam_width, nbest, max_labels, outs, workspace, lm=None, length_norm=False):
        """outs: (labels, lengths, scores), or with detail (labels, lengths, scores, label_frames, label_logps)"""
        B, T, J = enc.shape
        assert J == self.J, "enc: [B, T, J]"
        labels, lengths, scores = outs[:3]
        detail = len(outs) > 3
        check(*_rnnt_beam_entry("nntk_rnnt_beam_decode{}_device", lm, detail or length_norm,
                                (self.h, state, _dp(enc), B, T, _n_frames_ptr(n_frames, B), int(beam_width), int(nbest), int(max_labels)),
                                (lm.h if lm is not None else None,),
                                (_rnnt_beam_options(lm, length_norm, outs[3].data_ptr() if detail else None,
                                                    outs[4].data_ptr() if detail else None),),
                                (_ipv(labels), _ipv(lengths), _dp(scores), _dp(workspace))))
        return outs

    def beam_decode(self, enc, n_frames=None, beam_width=8, nbest=1, max_labels=None, lm=None, detail=False, length_norm=False):
        """``nntk_rnnt_beam_decode_device`` (INTEGRATION.md "RNN-Transducer: beam search"): enc [B, T, J] device tensor, n_frames host
        ints per row (None: T) -> (labels [B, nbest, max_labels] int32, -1 behind each hypothesis's labels; lengths [B, nbest] int32,
        -1 for a slot without a hypothesis; scores [B, nbest] float32, -inf there).  max_labels defaults to
        max_symbols_per_frame * T, which never truncates.  lm: an NgramLm fused into the search
        (``nntk_rnnt_beam_decode_lm_device``; scores then hold the model's terms and its end-of-sentence term), or None.
        detail: also return label_frames [B, nbest, max_labels] int32 (the frame each label was emitted in, -1 behind them) and
        label_logps, the same shape, float32 (the acoustic log-probability of each emission, 0 behind them): five tensors
        (``nntk_rnnt_beam_decode_opt_device``).  length_norm: the n-best is ordered by score / (length + 1); scores stay plain."""
        B, T, _ = enc.shape
        if max_labels is None:
            max_labels = max(1, self.max_symbols * T)
        outs = self._beam_outputs(enc.device, B, nbest, max_labels)
        if detail:
            outs = outs + self._beam_detail_outputs(enc.device, B, nbest, max_labels)
        return self._beam(None, enc, n_frames, beam_width, nbest, max_labels, outs,
                          self._beam_workspace(enc.device, B, beam_width, max_labels, lm, detail, length_norm), lm, length_norm)

    def destroy(self):
        if self.h:
            capi.load().nntk_rnnt_decoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class RnntGreedyStream:
    """``nntk_rnnt_decode_state_*``: greedy transducer decoding pushed chunk by chunk for ``batch`` independent streams.  After every
    push row b holds what ``decoder.decode`` gives on the row's frames since its last reset, bit for bit.  The stream owns the output
    buffers (labels, label_frames [batch, max_labels]; lengths, scores [batch]) and returns them from every push."""

    def __init__(self, decoder, batch, max_labels):
        self.dec, self.B, self.max_labels = decoder, int(batch), int(max_labels)
        self.outs = None
        self.h = capi.load().nntk_rnnt_decode_state_create(decoder.h, self.B)
        if not self.h:
            raise capi.NNTKError("nntk_rnnt_decode_state_create: " + capi.last_error())

    def push(self, enc_chunk, n_frames):
        """enc_chunk [batch, T, J] device tensor, n_frames host ints per row (0 allowed) -> (labels, label_frames, lengths, scores)"""
        assert enc_chunk.shape[0] == self.B, "enc_chunk: [batch, T, J]"
        if self.outs is None:
            self.outs = self.dec._outputs(enc_chunk.device, self.B, self.max_labels)
        return self.dec._decode(self.h, enc_chunk, n_frames, self.max_labels, self.outs)

    def reset(self, rows=None):
        """these rows (None: every row) start new streams"""
        _rnnt_state_reset("nntk_rnnt_decode_state_reset", self.h, rows)

    def close(self):
        if self.h:
            capi.load().nntk_rnnt_decode_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RnntBeamStream:
    """``nntk_rnnt_beam_state_*``: transducer beam search pushed chunk by chunk for ``batch`` independent streams.  After every push
    row b holds what ``decoder.beam_decode`` gives on the row's frames since its last reset, bit for bit.  The stream owns the output
    buffers (labels [batch, nbest, max_labels]; lengths, scores [batch, nbest]) and the workspace, and returns the outputs from every
    push.  lm: an NgramLm fused into the search (``nntk_rnnt_beam_state_create_lm``); it must stay open as long as the stream.
    detail: the stream also owns label_frames and label_logps [batch, nbest, max_labels] and every push returns five tensors, the
    frames counted from the start of each row's stream (``nntk_rnnt_beam_state_create_opt``).  length_norm: as in ``beam_decode``."""

    def __init__(self, decoder, batch, beam_width, nbest, max_labels, lm=None, detail=False, length_norm=False):
        self.dec, self.B, self.W, self.nbest, self.max_labels = decoder, int(batch), int(beam_width), int(nbest), int(max_labels)
        self.outs = self.ws = None
        self.lm, self.detail, self.length_norm = lm, bool(detail), bool(length_norm)
        lm_h = lm.h if lm is not None else None
        self.h, _ = _rnnt_beam_entry("nntk_rnnt_beam_state_create{}", lm, detail, (decoder.h, self.B, self.W, self.max_labels), (lm_h,), (lm_h, 1))
        if not self.h:
            raise capi.NNTKError("nntk_rnnt_beam_state_create: " + capi.last_error())

    def push(self, enc_chunk, n_frames):
        """enc_chunk [batch, T, J] device tensor, n_frames host ints per row (0 allowed) -> (labels, lengths, scores), with detail
        (labels, lengths, scores, label_frames, label_logps)"""
        assert enc_chunk.shape[0] == self.B, "enc_chunk: [batch, T, J]"
        if self.outs is None:
            self.outs = self.dec._beam_outputs(enc_chunk.device, self.B, self.nbest, self.max_labels)
            if self.detail:
                self.outs = self.outs + self.dec._beam_detail_outputs(enc_chunk.device, self.B, self.nbest, self.max_labels)
            self.ws = self.dec._beam_workspace(enc_chunk.device, self.B, self.W, self.max_labels, self.lm, self.detail, self.length_norm)
        return self.dec._beam(self.h, enc_chunk, n_frames, self.W, self.nbest, self.max_labels, self.outs, self.ws, self.lm,
                              self.length_norm)

    def reset(self, rows=None):
        """these rows (None: every row) start new streams"""
        _rnnt_state_reset("nntk_rnnt_beam_state_reset", self.h, rows)

    def close(self):
        if self.h:
            capi.load().nntk_rnnt_beam_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rnnt_host_decoder(embed, lstm_block, pred_proj, out, enc, max_labels, blank, joint_activation, max_symbols_per_frame):
    """the preamble of the numpy decode calls: the weights uploaded into a decoder of their own -> (decoder, enc as float32, B, T,
    max_labels with its default)"""
    import torch
    dev = lambda a: None if a is None else torch.from_numpy(_f32(a).reshape(-1) if a is not embed else _f32(a)).cuda()
    dec = RnntDecoder(dev(embed), dev(lstm_block), dev(pred_proj), dev(out), blank, joint_activation, max_symbols_per_frame)
    enc = _f32(enc)
    B, T, _ = enc.shape
    return dec, enc, B, T, max(1, dec.max_symbols * T) if max_labels is None else max_labels


def rnnt_beam_decode(embed, lstm_block, pred_proj, out, enc, n_frames=None, beam_width=8, nbest=1, max_labels=None, blank=0,
                     joint_activation=ACT_TANH, max_symbols_per_frame=10, lm=None, detail=False, length_norm=False):
    """Transducer beam search on numpy arrays (the weights go to the device, ``nntk_rnnt_beam_decode`` takes enc and the results as
    host memory): enc [B, T, J] -> (labels [B, nbest, max_labels], lengths [B, nbest], scores [B, nbest]).  lm: an NgramLm fused into
    the search (``nntk_rnnt_beam_decode_lm``), or None.  detail, length_norm: as in ``RnntDecoder.beam_decode``
    (``nntk_rnnt_beam_decode_opt``; with detail label_frames and label_logps follow the scores)."""
    dec, enc, B, T, max_labels = _rnnt_host_decoder(embed, lstm_block, pred_proj, out, enc, max_labels, blank, joint_activation,
                                                    max_symbols_per_frame)
    labels = np.empty((B, nbest, max_labels), np.int32)
    lengths, scores = np.empty((B, nbest), np.int32), np.empty((B, nbest), np.float32)
    frames, logps = (np.empty(labels.shape, np.int32), np.empty(labels.shape, np.float32)) if detail else (None, None)
    try:
        check(*_rnnt_beam_entry("nntk_rnnt_beam_decode{}", lm, detail or length_norm,
                                (dec.h, None, _p(enc), B, T, _n_frames_ptr(n_frames, B), int(beam_width), int(nbest), int(max_labels)),
                                (lm.h if lm is not None else None,),
                                (_rnnt_beam_options(lm, length_norm, frames.ctypes.data if detail else None,
                                                    logps.ctypes.data if detail else None),),
                                (labels.ctypes.data_as(capi.ip), lengths.ctypes.data_as(capi.ip), _p(scores))))
    finally:
        dec.destroy()
    return (labels, lengths, scores, frames, logps) if detail else (labels, lengths, scores)


def rnnt_greedy_decode(embed, lstm_block, pred_proj, out, enc, n_frames=None, max_labels=None, blank=0, joint_activation=ACT_TANH,
                       max_symbols_per_frame=10):
    """Greedy transducer decoding on numpy arrays (the weights go to the device, ``nntk_rnnt_greedy_decode`` takes enc and the results
    as host memory): enc [B, T, J] -> (labels [B, max_labels], label_frames, lengths [B], scores [B])"""
    dec, enc, B, T, max_labels = _rnnt_host_decoder(embed, lstm_block, pred_proj, out, enc, max_labels, blank, joint_activation,
                                                    max_symbols_per_frame)
    labels, frames = np.empty((B, max_labels), np.int32), np.empty((B, max_labels), np.int32)
    lengths, scores = np.empty(B, np.int32), np.empty(B, np.float32)
    try:
        check(capi.load().nntk_rnnt_greedy_decode(dec.h, None, _p(enc), B, T, _n_frames_ptr(n_frames, B), int(max_labels),
                                                  labels.ctypes.data_as(capi.ip), frames.ctypes.data_as(capi.ip),
                                                  lengths.ctypes.data_as(capi.ip), _p(scores)), "nntk_rnnt_greedy_decode")
    finally:
        dec.destroy()
    return labels, frames, lengths, scores


def _host_ids(ids):
    return np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))


def embedding_lookup_device(table, ids, out=None):
    """``nntk_embedding_lookup_device``: table [V, E] device tensor, ids host ints (-1: a row of zeros) -> out [len(ids), E], bit copies of
    the table's rows"""
    V, E = table.shape
    idv = _host_ids(ids)
    rows = idv.shape[0]
    if out is None:
        out = table.new_empty((rows, E))
    assert out.numel() == rows * E, "out: [rows, E]"
    check(capi.load().nntk_embedding_lookup_device(_dp(table), V, E, idv.ctypes.data_as(capi.ip), rows, _dp(out) if rows else None),
          "nntk_embedding_lookup_device")
    return out


def embedding_gradient_device(dout, ids, V, dtable=None, workspace=None):
    """``nntk_embedding_gradient_device``: dout [rows, E] device tensor, ids host ints -> dtable [V, E], overwritten: the sum of the rows of
    each id, exact zeros for an absent id; rows with id -1 are never read.  No atomics, the same bits on every call."""
    import torch
    idv = _host_ids(ids)
    rows = idv.shape[0]
    E = dout.shape[-1]
    assert dout.numel() == rows * E, "dout: [rows, E]"
    L = capi.load()
    need = L.nntk_embedding_workspace_floats(rows, V, E)
    if dtable is None:
        dtable = dout.new_empty((V, E))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=dout.device)
    assert dtable.numel() == V * E, "dtable: [V, E]"
    assert workspace.numel() >= need, "workspace: nntk_embedding_workspace_floats(rows, V, E) floats"
    check(L.nntk_embedding_gradient_device(_dp(dout) if rows else None, idv.ctypes.data_as(capi.ip), rows, V, E, _dp(dtable), _dp(workspace)),
          "nntk_embedding_gradient_device")
    return dtable


class RnntPredictor:
    """``nntk_rnnt_predictor_*``: the decoder's prediction network -- label embedding, one LSTM, a linear projection (proj=False: the
    identity, H == J) -- in training, on the device blocks ``RnntDecoder`` takes (INTEGRATION.md "RNN-Transducer: training the prediction
    network").  forward gives pred [batch, max_label_len + 1, J] for the loss calls, backward the gradients of the three blocks."""

    def __init__(self, V, E, H, J, batch, max_label_len, blank=0, proj=True):
        self.V, self.E, self.H, self.J, self.batch, self.max_label_len = int(V), int(E), int(H), int(J), int(batch), int(max_label_len)
        self.has_proj = bool(proj)
        cfg = capi.NntkRnntPredictorConfig(self.V, self.E, self.H, self.J, int(blank), int(self.has_proj), self.batch, self.max_label_len)
        self.h = capi.load().nntk_rnnt_predictor_create(cfg)
        if not self.h:
            raise capi.NNTKError("nntk_rnnt_predictor_create: " + capi.last_error())

    def load_weights(self, embed, lstm_block, pred_proj):
        """``nntk_rnnt_predictor_load_weights_device``: embed [V, E], the flat LSTM block, the flat projection block (None without one);
        the handle keeps copies, so call it again after every optimizer step"""
        check(capi.load().nntk_rnnt_predictor_load_weights_device(self.h, _dp(embed), _dp(lstm_block),
                                                                  _dp(pred_proj) if pred_proj is not None else None),
              "nntk_rnnt_predictor_load_weights_device")

    def forward(self, labels, label_lengths=None, pred=None):
        """labels: a list of per-row lists, or a padded int array [batch, max_label_len] with label_lengths (as ``rnnt_loss_device``)
        -> pred [batch, max_label_len + 1, J]; rows u > label_lengths[b] hold the projection's bias"""
        import torch
        lab, ll = _rnnt_labels(labels, label_lengths, self.batch, self.max_label_len)
        if pred is None:
            pred = torch.empty((self.batch, self.max_label_len + 1, self.J), dtype=torch.float32, device="cuda")
        assert pred.numel() == self.batch * (self.max_label_len + 1) * self.J, "pred: [batch, max_label_len + 1, J]"
        check(capi.load().nntk_rnnt_predictor_forward_device(self.h, lab.ctypes.data_as(capi.ip), ll.ctypes.data_as(capi.ip), _dp(pred)),
              "nntk_rnnt_predictor_forward_device")
        return pred

    def backward(self, dpred, dembed=None, dlstm=None, dproj=None):
        """dpred [batch, max_label_len + 1, J] (rows u > label_lengths[b] are ignored) -> (dembed [V, E], dlstm, dproj or None), all
        overwritten; pass the gradient tensors registered with ``Optimizer`` to have them filled in place"""
        if dembed is None:
            dembed = dpred.new_empty((self.V, self.E))
        if dlstm is None:
            dlstm = dpred.new_empty(4 * self.H * (self.E + self.H + 2))
        if dproj is None and self.has_proj:
            dproj = dpred.new_empty((self.H + 1) * self.J)
        assert dpred.numel() == self.batch * (self.max_label_len + 1) * self.J, "dpred: [batch, max_label_len + 1, J]"
        assert dembed.numel() == self.V * self.E and dlstm.numel() == 4 * self.H * (self.E + self.H + 2), "dembed [V, E], dlstm: the flat block"
        assert dproj is None or dproj.numel() == (self.H + 1) * self.J, "dproj: the flat block W [H,J] | b [J]"
        check(capi.load().nntk_rnnt_predictor_backward_device(self.h, _dp(dpred), _dp(dembed), _dp(dlstm),
                                                              _dp(dproj) if dproj is not None else None),
              "nntk_rnnt_predictor_backward_device")
        return dembed, dlstm, dproj

    def device_bytes(self):
        return int(capi.load().nntk_rnnt_predictor_device_bytes(self.h))

    def destroy(self):
        if self.h:
            capi.load().nntk_rnnt_predictor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class LSTM(_Recurrent):
    def __init__(self, in_features, hidden, return_sequences, timesteps, v2=True, acts=None, mini_batch=None):
        L = capi.load()
        self.acts = L.LSTMActivationsCreateDefault(hidden) if acts is None else acts
        self.cfg = L.LSTMConfigCreate(in_features, hidden, return_sequences, timesteps, v2, self.acts)
        # mini_batch: a *CreateForTraining handle of that mini-batch size (the training calls), else an inference handle
        self.mini_batch = mini_batch
        self.h = (L.LSTMCreateForTraining(self.cfg, capi.ConvTrainingConfig(mini_batch)) if mini_batch else
                  L.LSTMCreateForInference(self.cfg))
        self._get_weights, self._apply, self._apply_batch = L.LSTMGetWeights, L.LSTMApplyInference, L.LSTMApplyInferenceBatch
        self._apply_device, self._sync, self._reset = L.LSTMApplyDevice, L.LSTMSyncWeights, L.LSTMResetState
        self._apply_device_vl, self._is_lstm = L.LSTMApplyDeviceVarLen, True
        self._destroy, self._acts_destroy = L.LSTMDestroy, L.LSTMActivationsDestroy

    def state(self):
        H = self.cfg.base.output_feature_channels
        h, c = np.empty(H, np.float32), np.empty(H, np.float32)
        check(capi.load().LSTMGetState(self.h, _p(h), _p(c)), "LSTMGetState")
        return h, c


class TimeDistributedDense:
    def __init__(self, ts, in_features, out_features, act=None):
        L = capi.load()
        self.act = act
        dense = L.DenseConfigCreate(in_features, out_features, act.h if act else None)
        self.cfg = L.TimeDistributedDenseConfigCreate(ts, dense)
        self.h = L.TimeDistributedDenseCreateForInference(self.cfg)

    def set_weights(self, W, b):
        w = capi.load().TimeDistributedDenseGetWeights(self.h).contents
        _fill(w.W, W)
        _fill(w.b, b)

    def apply(self, x):
        x = _f32(x)
        L = capi.load()
        ts, out = self.cfg.ts, self.cfg.dense.output_size
        if x.ndim == 2:
            o = np.empty((ts, out), np.float32)
            check(L.TimeDistributedDenseApplyInference(self.h, _p(x), _p(o)), "TimeDistributedDenseApplyInference")
        else:
            o = np.empty((x.shape[0], ts, out), np.float32)
            check(L.TimeDistributedDenseApplyInferenceBatch(self.h, _p(x), _p(o), x.shape[0]),
                  "TimeDistributedDenseApplyInferenceBatch")
        return o

    def apply_device(self, x, out=None):
        if out is None:
            out = x.new_empty((x.shape[0], self.cfg.ts, self.cfg.dense.output_size))
        check(capi.load().TimeDistributedDenseApplyDevice(self.h, _dp(x), _dp(out), x.shape[0]),
              "TimeDistributedDenseApplyDevice")
        return out

    def apply_device_varlen(self, x, lengths=None, out=None):
        """TimeDistributedDenseApplyDeviceVarLen: rows t >= lengths[b] of the output are zeros"""
        B = x.shape[0]
        if tuple(x.shape[1:]) != (self.cfg.ts, self.cfg.dense.input_size):
            raise ValueError("TimeDistributedDenseApplyDeviceVarLen: input must be [B, %d, %d]" % (self.cfg.ts, self.cfg.dense.input_size))
        if out is None:
            out = x.new_empty((B, self.cfg.ts, self.cfg.dense.output_size))
        elif tuple(out.shape) != (B, self.cfg.ts, self.cfg.dense.output_size):
            raise ValueError("TimeDistributedDenseApplyDeviceVarLen: out must be [B, %d, %d]" % (self.cfg.ts, self.cfg.dense.output_size))
        lp = None
        if lengths is not None:
            lens = _host_ints(lengths, B, "lengths")
            lp = lens.ctypes.data_as(capi.ip)
        check(capi.load().TimeDistributedDenseApplyDeviceVarLen(self.h, _dp(x), _dp(out), B, lp), "TimeDistributedDenseApplyDeviceVarLen")
        return out

    def load_weights_device(self, block):
        """TimeDistributedDenseLoadWeightsDevice: the GetWeights() block from a device tensor (same order and size), then what sync_weights does"""
        check(capi.load().TimeDistributedDenseLoadWeightsDevice(self.h, _dp(block)), "TimeDistributedDenseLoadWeightsDevice")

    def destroy(self):
        if self.h:
            capi.load().TimeDistributedDenseDestroy(self.h)
            self.h = None


class Dense:
    def __init__(self, in_features, out_features, act=None):
        L = capi.load()
        self.act = act
        self.cfg = L.DenseConfigCreate(in_features, out_features, act.h if act else None)
        self.h = L.DenseCreateForInference(self.cfg)

    def set_weights(self, W, b):
        w = capi.load().DenseGetWeights(self.h).contents
        _fill(w.W, W)
        _fill(w.b, b)

    def apply(self, x):
        x = _f32(x)
        o = np.empty(self.cfg.output_size, np.float32)
        check(capi.load().DenseApplyInference(self.h, _p(x), _p(o)), "DenseApplyInference")
        return o

    def load_weights_device(self, block):
        """DenseLoadWeightsDevice: the GetWeights() block from a device tensor (same order and size), then what sync_weights does"""
        check(capi.load().DenseLoadWeightsDevice(self.h, _dp(block)), "DenseLoadWeightsDevice")

    def destroy(self):
        if self.h:
            capi.load().DenseDestroy(self.h)
            self.h = None


_OPTIMIZER_KINDS = {"sgd": 0, "momentum": 1, "adam": 2}


class Optimizer:
    """``nntk_optimizer_*``: one device-side step over a list of (weights, gradient) device tensors -- SGD ("sgd"), momentum SGD
    ("momentum") or Adam / AdamW ("adam", AdamW with weight_decay and decoupled=True) with PyTorch's semantics, gradient scaling,
    global-norm clipping, the non-finite guard and gradient zeroing in two launches.  Keyword arguments are the fields of
    NntkOptimizerConfig (learning_rate, momentum, nesterov, beta1, beta2, epsilon, weight_decay, decoupled, grad_scale, clip_norm,
    zero_gradients); "adam" defaults to PyTorch's beta1 = 0.9, beta2 = 0.999, epsilon = 1e-8.  The tensors are kept alive by the object."""

    def __init__(self, kind, blocks, **cfg):
        k = _OPTIMIZER_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
        if isinstance(k, str):
            raise ValueError("Optimizer: kind must be one of %s" % sorted(_OPTIMIZER_KINDS))
        if k == 2:
            cfg = dict({"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8}, **cfg)
        c = capi.NntkOptimizerConfig(kind=k)
        names = {f for f, _ in capi.NntkOptimizerConfig._fields_} - {"kind"}
        for key, value in cfg.items():
            if key not in names:
                raise TypeError("Optimizer: unknown option %r" % key)
            setattr(c, key, value)
        self.blocks = [(w, g) for w, g in blocks]
        for w, g in self.blocks:
            assert w.numel() == g.numel(), "Optimizer: a gradient has the size of its weights"
            if w.numel():
                _dp(w), _dp(g)
        n = len(self.blocks)
        wp = (C.c_void_p * max(n, 1))(*[w.data_ptr() if w.numel() else None for w, _ in self.blocks])
        gp = (C.c_void_p * max(n, 1))(*[g.data_ptr() if g.numel() else None for _, g in self.blocks])
        sz = (C.c_long * max(n, 1))(*[w.numel() for w, _ in self.blocks])
        self.cfg, self.kind = c, k
        self.h = capi.load().nntk_optimizer_create(c, n, wp, gp, sz)
        if not self.h:
            raise capi.NNTKError("nntk_optimizer_create: " + capi.last_error())

    def step(self):
        """nntk_optimizer_step_device on the current stream: asynchronous, nothing is read back"""
        check(capi.load().nntk_optimizer_step_device(self.h), "nntk_optimizer_step_device")

    def set_learning_rate(self, lr):
        check(capi.load().nntk_optimizer_set_learning_rate(self.h, C.c_float(lr)), "nntk_optimizer_set_learning_rate")

    def _download(self, ptr, n):
        out = np.empty(n, np.float32)
        if n:
            check(capi.load().nntk_device_download(_p(out), C.c_void_p(ptr), n), "nntk_device_download")
        return out

    def info(self):
        """a host copy (this waits for the stream) of [norm before clipping, clip factor applied, 1.0 if the step was skipped, steps taken]"""
        return self._download(capi.load().nntk_optimizer_info_device(self.h), 4)

    def state(self, block):
        """host copies (m, v) of one block's moments, None where the kind has none: for checkpoints"""
        m, v = C.c_void_p(), C.c_void_p()
        check(capi.load().nntk_optimizer_state_device(self.h, block, C.byref(m), C.byref(v)), "nntk_optimizer_state_device")
        n = self.blocks[block][0].numel()
        return tuple(self._download(q.value, n).reshape(tuple(self.blocks[block][0].shape)) if q.value else None for q in (m, v))

    def destroy(self):
        if self.h:
            capi.load().nntk_optimizer_destroy(self.h)
            self.h = None


_WINDOWS = ("ones", "hann_window", "hamming_window", "periodic_hann_window", "periodic_hamming_window",
            "blackman_window")


def window(name, size):
    assert name in _WINDOWS
    v = np.empty(size, np.float32)
    getattr(capi.load(), name)(_p(v), size)
    return v


class Spectrogram:
    def __init__(self, nfft, window_size, noverlap, input_size, mode="magnitude", fs=16000, fft_norm=1.0,
                 window_name="hann_window"):
        L = capi.load()
        self.cfg = L.SpectrogramConfigCreate(nfft, window_size, noverlap, input_size, C.c_float(fft_norm))
        self.h = L.SpectrogramCreateMagnitude(self.cfg) if mode == "magnitude" else L.SpectrogramCreatePSD(self.cfg, fs)
        if window_name:
            L.SpectrogramSetWindowFunc(self.h, C.cast(getattr(L, window_name), C.c_void_p))

    @property
    def out_shape(self):
        return (self.cfg.ntime_series, self.cfg.nfreq)

    def apply(self, x):
        x = _f32(x)
        L = capi.load()
        if x.ndim == 1:
            out = np.full(self.out_shape, np.nan, np.float32)
            L.SpectrogramApply(self.h, _p(x), _p(out))
            if capi.last_error():
                raise capi.NNTKError(capi.last_error())
        else:
            out = np.empty((x.shape[0],) + self.out_shape, np.float32)
            check(L.SpectrogramApplyBatch(self.h, _p(x), _p(out), x.shape[0]), "SpectrogramApplyBatch")
        return out

    def apply_device(self, x, out=None):
        if out is None:
            out = x.new_empty((x.shape[0],) + self.out_shape)
        check(capi.load().SpectrogramApplyDevice(self.h, _dp(x), _dp(out), x.shape[0]), "SpectrogramApplyDevice")
        return out

    def stream_sizes(self):
        """(tail_floats, max_frames): nntk_spectrogram_stream_sizes"""
        a, b = C.c_int(), C.c_int()
        check(capi.load().nntk_spectrogram_stream_sizes(self.cfg, C.byref(a), C.byref(b)), "nntk_spectrogram_stream_sizes")
        return a.value, b.value

    @property
    def stream_features(self):
        return self.cfg.nfreq

    def new_stream_state(self, batch):
        """(tail [batch, tail_floats] zeros on the current device, host int32 tail_len [batch] zeros)"""
        import torch
        tf, _ = self.stream_sizes()
        return (torch.zeros((batch, tf), device="cuda"), np.zeros(batch, np.int32))

    def apply_device_stream(self, x, n_new, state, final=None, out=None):
        """SpectrogramApplyDeviceStream: x [B, input_size] chunk samples, row b brings n_new[b] of them.
        Returns (out [B, max_frames, nfreq], frames); the state (tail tensor, tail_len) is updated in place."""
        tf, mf = self.stream_sizes()
        return _stream_call(capi.load().SpectrogramApplyDeviceStream, "SpectrogramApplyDeviceStream", (self.h,), x,
                            (self.cfg.input_size,), n_new, state, (tf,), final, (x.shape[0], mf, self.cfg.nfreq), out)

    def destroy(self):
        if self.h:
            capi.load().SpectrogramDestroy(self.h)
            self.h = None


class LogMelSpectrogram:
    """LogMelSpectrogramCreate over a Spectrogram (owned by the caller, as in the reference): log(mel + 1.5849e-13)"""

    def __init__(self, spectrogram, n_mels, sample_rate=16000, lower_hz=0.0, upper_hz=8000.0):
        L = capi.load()
        self.spec = spectrogram
        self.mel_cfg = L.MelFilterBankConfigCreate(n_mels, spectrogram.cfg.nfft, sample_rate, C.c_float(lower_hz), C.c_float(upper_hz))
        self.h = L.LogMelSpectrogramCreate(spectrogram.h, self.mel_cfg)
        if not self.h:
            raise capi.NNTKError("LogMelSpectrogramCreate: " + capi.last_error())
        self.cfg = spectrogram.cfg

    @property
    def out_shape(self):
        return (self.cfg.ntime_series, self.mel_cfg.n_mels)

    @property
    def stream_features(self):
        return self.mel_cfg.n_mels

    def apply_device(self, x, out=None):
        if out is None:
            out = x.new_empty((x.shape[0],) + self.out_shape)
        check(capi.load().LogMelSpectrogramApplyDevice(self.h, _dp(x), _dp(out), x.shape[0]), "LogMelSpectrogramApplyDevice")
        return out

    def stream_sizes(self):
        return self.spec.stream_sizes()

    def new_stream_state(self, batch):
        return self.spec.new_stream_state(batch)

    def apply_device_stream(self, x, n_new, state, final=None, out=None):
        """LogMelSpectrogramApplyDeviceStream: as Spectrogram.apply_device_stream, output [B, max_frames, n_mels]"""
        tf, mf = self.stream_sizes()
        return _stream_call(capi.load().LogMelSpectrogramApplyDeviceStream, "LogMelSpectrogramApplyDeviceStream", (self.h,), x,
                            (self.cfg.input_size,), n_new, state, (tf,), final, (x.shape[0], mf, self.mel_cfg.n_mels), out)

    def destroy(self):
        if self.h:
            capi.load().LogMelSpectrogramDestroy(self.h)
            self.h = None
