"""Chunked streaming through the whole stack: Spectrogram (or LogMelSpectrogram) -> Conv1d(+BN+act) stages -> GRU / LSTM / RNN
layers -> optional TimeDistributedDense, for B independent streams at once (INTEGRATION.md "Streaming a whole stack").

Every stage carries what the next chunk needs in a device buffer: the spectrogram's sample tail and each conv's input history
(``*ApplyDeviceStream``, updated in place), the recurrent layers' h / c (``*ApplyDeviceVarLen``, double-buffered).  The frames a
row emits have the bits of the one-shot per-layer chain on that row's whole stream.  No arithmetic happens here; zeroing state
rows of a finished stream is torch plumbing.
"""
import numpy as np

from . import layers as NL


class StreamingStack:
    """push(x, n_new, final) runs one chunk for every row through every stage.

    frontend:          layers.Spectrogram or layers.LogMelSpectrogram; its input_size = the most samples a row brings per push
    conv_stages:       list of Conv1d or (Conv1d, BatchNorm or None, Activation or None); conv i's input_size = the previous stage's
                       max frames / outputs, its input channels = the previous stage's features
    recurrent_layers:  GRU / LSTM / RNN with return_sequences=True, timesteps = the last conv's max_outputs
    head:              optional TimeDistributedDense with ts = that same length
    """

    def __init__(self, frontend, conv_stages, recurrent_layers, head=None, batch=1):
        import torch
        self.B = int(batch)
        self.frontend = frontend
        self.convs = [(c, None, None) if isinstance(c, NL.Conv1d) else tuple(c) + (None,) * (3 - len(c)) for c in conv_stages]
        self.rec = list(recurrent_layers)
        self.head = head
        _, T = frontend.stream_sizes()
        feat = frontend.stream_features
        for i, (conv, bn, _) in enumerate(self.convs):
            if conv.cfg.input_size != T or conv.cfg.input_feature_channels != feat:
                raise ValueError("conv stage %d: input_size %d / channels %d, the previous stage gives %d / %d"
                                 % (i, conv.cfg.input_size, conv.cfg.input_feature_channels, T, feat))
            _, T = conv.stream_sizes()
            feat = conv.cfg.output_feature_channels
        for i, r in enumerate(self.rec):
            base = r.cfg.base
            if not base.return_sequences:
                raise ValueError("recurrent layer %d must return sequences" % i)
            if base.timesteps != T or base.input_feature_channels != feat:
                raise ValueError("recurrent layer %d: timesteps %d / input %d, the previous stage gives %d / %d"
                                 % (i, base.timesteps, base.input_feature_channels, T, feat))
            feat = base.output_feature_channels
        if head is not None and (head.cfg.ts != T or head.cfg.dense.input_size != feat):
            raise ValueError("head: ts %d / input %d, the previous stage gives %d / %d" % (head.cfg.ts, head.cfg.dense.input_size, T, feat))
        self.T_cap = T
        self.front_state = frontend.new_stream_state(self.B)
        self.conv_states = [conv.new_stream_state(self.B) for conv, _, _ in self.convs]
        z = lambda r: torch.zeros((self.B, r.cfg.base.output_feature_channels), device="cuda")
        # [current, spare] per layer: a call reads h0 from one and writes hT into the other, then they swap
        self.h = [[z(r), z(r)] for r in self.rec]
        self.c = [[z(r), z(r)] if r._is_lstm else None for r in self.rec]

    def reset(self, rows):
        """empty the state of these rows: the slots start new streams"""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.size == 0:
            return
        import torch
        idx = torch.as_tensor(rows, device="cuda")
        tail, tl = self.front_state
        tail[idx] = 0
        tl[rows] = 0
        for hist, hl in self.conv_states:
            hist[idx] = 0
            hl[rows] = 0
        for i in range(len(self.rec)):
            self.h[i][0][idx] = 0
            if self.c[i] is not None:
                self.c[i][0][idx] = 0

    def push(self, x, n_new, final=None):
        """x: [B, frontend input_size] samples, row b's first n_new[b] are new.  Returns (out [B, T_cap, C], counts): row b's new
        frames, zeros past counts[b].  Rows marked final emit their held-back frame and start empty on the next push."""
        out, cnt = self.frontend.apply_device_stream(x, n_new, self.front_state, final=final)
        for (conv, bn, act), st in zip(self.convs, self.conv_states):
            out, cnt = conv.apply_device_stream(out, cnt, st, bn=bn, act=act, final=final)
        for i, r in enumerate(self.rec):
            h0, hT = self.h[i]
            if r._is_lstm:
                c0, cT = self.c[i]
                out, _, _ = r.apply_device_varlen(out, cnt, h0=h0, c0=c0, return_state=True, hT=hT, cT=cT)
                self.c[i].reverse()
            else:
                out, _ = r.apply_device_varlen(out, cnt, h0=h0, return_state=True, hT=hT)
            self.h[i].reverse()
        if self.head is not None:
            out = self.head.apply_device_varlen(out, cnt)
        if final is not None and self.rec:
            done = np.nonzero(np.asarray(final).reshape(-1))[0]
            if done.size:
                import torch
                idx = torch.as_tensor(done, device="cuda")
                for i in range(len(self.rec)):
                    self.h[i][0][idx] = 0
                    if self.c[i] is not None:
                        self.c[i][0][idx] = 0
        return out, cnt
