"""The host plan of a token step, shared by the two host-planned token loaders: ``ZeroCopyTokenLoader`` and
``ResidentTokenLoader`` (whose ``plan="device"`` mode shares the construction and nothing of the slot ring).

Per step the host does O(local batch) work and touches no token: this rank's indices of the world-size-invariant
``EpochOrder``, the sequence lengths from the corpus offsets, the FFD rule, the native ``pack_plan`` -- written as
one ``TokenWindowLayout(k=1)`` header behind a descriptor (``src_start [LB] i64`` and one array the subclass
declares) into a slot of a small pinned ring, which the subclass copies to the device and launches from. With
``device="cpu"`` the slot is the window itself, and the batch is the host ``gather_ragged`` + the host collate.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _native
from .models.tokens import (META_FIELDS, SharedTokenSource, TokenWindowLayout, collate_token_window,
                            ffd_if_it_wins)
from .ops.kernels import check_ignore_index
from .permutation import EpochOrder
from .resident import PrefetchedIndexedLoader
from .types import DDLEnv
from .utils import streams


class HostPlannedTokenLoader(PrefetchedIndexedLoader):
    def __init__(self, source: SharedTokenSource, global_batch: int, seq_len: int, mode: str, env: DDLEnv | None, *,
                 seed: int, pack_order: str, token_rows: str, pad_id: int, depth: int,
                 device: str | torch.device | None, n_epochs: int | None, resume_state: dict | None, handoff: str,
                 labels: bool = False, ignore_index: int = -100):
        """The construction the loaders share. The options are checked (``check_token_options``) by the subclass,
        in front of its own rules. ``labels``: every batch gains ``"labels"``, the next-token targets
        (``ops.ref_token_labels``) with ``ignore_index`` where there is none, written by the kernel that writes the
        batch; nothing else of the loader (order, checkpoint, stats) depends on it."""
        self.labels, self.ignore_index = bool(labels), check_ignore_index(labels, ignore_index)
        self.handoff = handoff
        self.env = env or DDLEnv()
        self.W, self.rank = self.env.world_size, self.env.rank
        self.source, self.seq_len, self.mode = source, int(seq_len), mode
        self.pack_order, self.token_rows, self.pad_id = pack_order, token_rows, int(pad_id)
        self.order = EpochOrder(source.n, global_batch, seed)
        self.GB, self.LB = int(global_batch), self.order.local_batch(self.W)
        self.out_dtype = torch.int32  # input_ids (the checkpoint's dtype field)
        self.device = self._resolve_device(self.env, device)
        self._init_cursor(seed, depth, n_epochs, resume_state)

        lay = self.layout = TokenWindowLayout(self.LB, self.seq_len, source.max_len, 1, source.token_bytes)
        self._reg = lay.regions()
        self._hdr_bytes = self._reg["tokens"][0]  # meta + header arrays: everything in front of the tokens
        # in front of the header: the descriptor, src_start [LB] i64 + the subclass's array
        _, dtype, count = self._desc_extra()
        self._desc_bytes = -(-(8 * self.LB + np.dtype(dtype).itemsize * count) // 16) * 16
        self._toks = source.tokens.tensor().view(-1)  # keeps the mappings alive
        self._offs_t = source.offsets.tensor().view(-1)
        self._offs = self._offs_t.numpy()
        self.nbytes = int(self._offs[-1]) * source.token_bytes if source.n else 0
        self.prep_stream = streams.batch_stream(self.device) if self.device.type == "cuda" else None
        self._windows: list = []

    def _desc_extra(self) -> tuple:
        """(name, numpy dtype, count) of the descriptor array behind ``src_start``."""
        raise NotImplementedError

    def _init_ring(self, window_bytes: int) -> None:
        """``depth + 1`` windows of ``window_bytes`` on the device and the host buffers the plans are written
        into. On the GPU those are pinned slots (descriptor + header), one more than the windows: a slot is
        rewritten only after the copy out of it has completed (its event), which is normally long done. The
        CPU twin writes the header straight into the window."""
        self._windows = [torch.empty(window_bytes, dtype=torch.uint8, device=self.device)
                         for _ in range(self.depth + 1)]
        if self.prep_stream is not None:
            self._slots = [torch.empty(self._desc_bytes + self._hdr_bytes, dtype=torch.uint8, pin_memory=True)
                           for _ in range(self.depth + 2)]
            self._slot_ev = [None] * len(self._slots)
        else:
            self._slots = self._windows
        self._views = [self._host_views(b) for b in self._slots]

    def _host_views(self, buf: torch.Tensor) -> dict:
        """numpy views (and raw addresses) of the descriptor and header arrays at the front of a host buffer."""
        a = buf.numpy()
        d, LB = self._desc_bytes, self.LB
        name, dtype, count = self._desc_extra()
        v = {"src_start": a[:8 * LB].view(np.int64),
             name: a[8 * LB:8 * LB + np.dtype(dtype).itemsize * count].view(dtype)}
        for key in ("meta", "offsets", "row_start", "row_end", "seg_offsets"):
            off, count = self._reg[key]
            v[key] = a[d + off:d + off + 8 * count].view(np.int64)
        v["ptr"] = {k: int(x.ctypes.data) for k, x in v.items()}
        return v

    def _plan(self, t: int) -> tuple:
        """Write step ``t``'s descriptor and header into its slot. Returns (slot index, the slot's views, the
        batch's corpus indices, meta = (n_tokens, n_rows, n_seg, max_seg, 0))."""
        e, g = divmod(t, self.order.batches_per_epoch)
        offs = self._offs
        idx = np.asarray(self.order.indices(e, g, self.rank, self.W), dtype=np.int64)
        lens = offs[idx + 1] - offs[idx]
        pack = self.mode == "pack"
        if pack and self.pack_order == "ffd":
            order = ffd_if_it_wins(lens, self.seq_len)
            if order is not None:
                idx, lens = idx[order], lens[order]
        k = t % len(self._slots)
        if self.prep_stream is not None and self._slot_ev[k] is not None and not self._slot_ev[k].query():
            self._slot_ev[k].synchronize()  # the H2D copy out of this slot (depth + 2 batches ago)
        v = self._views[k]
        p = v["ptr"]
        v["src_start"][:] = offs[idx]
        v["offsets"][0] = 0
        np.cumsum(lens, out=v["offsets"][1:])
        n_tokens = int(v["offsets"][self.LB])
        if n_tokens > self._reg["tokens"][1]:
            raise ValueError(f"{n_tokens} tokens exceed the window's {self._reg['tokens'][1]}: the corpus holds a "
                             "sequence longer than source.max_len")
        n_rows = n_seg = max_seg = 0
        if pack:
            cap = self.layout.max_segments
            n_rows, n_seg = _native.runtime().pack_plan(p["offsets"], self.LB, self.seq_len, p["row_start"],
                                                        p["row_end"], cap, p["seg_offsets"], cap)
            if n_seg:
                max_seg = int(np.diff(v["seg_offsets"][: n_seg + 1]).max())
        meta = (n_tokens, n_rows, n_seg, max_seg, 0)
        v["meta"][:META_FIELDS] = meta
        return k, v, idx, meta

    def _upload(self, hip, k: int, win: torch.Tensor) -> None:
        """Slot ``k`` (descriptor + header) to the front of the device window, on the prep stream (``hip``: the
        caller's ``_native.hip()``, fetched once per step)."""
        st = self.prep_stream
        hip.memcpy_h2d(win.data_ptr(), self._slots[k].data_ptr(), self._desc_bytes + self._hdr_bytes, st.cuda_stream)
        if self._slot_ev[k] is None:
            self._slot_ev[k] = torch.cuda.Event()
        self._slot_ev[k].record(st)

    def _cpu_batch(self, t: int, v: dict, idx: np.ndarray, meta: tuple) -> dict:
        """The CPU twin: the host ``gather_ragged`` behind the header just written, and the host collate."""
        win = self._windows[t % len(self._windows)]
        _native.runtime().gather_ragged(win.data_ptr() + self._desc_bytes + self._hdr_bytes, v["ptr"]["offsets"],
                                        self._toks.data_ptr(), self._offs_t.data_ptr(), self.source.n, idx,
                                        self.source.token_bytes, self._reg["tokens"][1], 2)
        return collate_token_window(win[self._desc_bytes:], self.layout, self.mode, meta, self.pad_id,
                                    fixed_rows=self.token_rows == "fixed", labels=self.labels,
                                    ignore_index=self.ignore_index)

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass
