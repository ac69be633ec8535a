"""Producer-free zero-copy token loader (BASELINE config 4): the ragged gather kernel packs every batch's
sequences straight out of the pinned, device-mapped corpus.

``TokenBatchProducer`` gathers each batch on the host into a pinned window (a DRAM read and a streaming-store
write of every token) that the GPU then DMA-reads: three socket-DRAM passes per token. Here the corpus (node
shm) is registered once, page-rounded, and per step

* the host does O(local batch) work and touches no token: this rank's indices of the world-size-invariant
  ``EpochOrder``, the sequence lengths from the corpus offsets, the producer's FFD rule, the native
  ``pack_plan`` -- written as one ``TokenWindowLayout(k=1)`` header plus the gather's descriptor
  (``src_start``, ``tile_start``) into a slot of a small pinned ring;
* the prep stream copies that header into a device window (one small H2D), the ``gather_ragged`` gfx950
  kernel fills the window's tokens region over PCIe (16-byte aligned loads of each sequence's aligned hull,
  grid capped by ``max_blocks``), and the unchanged ``collate_token_window`` expands the window.

The device window holds exactly the bytes the producer's window would hold, so the batches are identical to
the producer path's, key by key. One DRAM pass per token, no producers, no host copy. The order and the
``kind="indexed"`` checkpoint are ``PrefetchedIndexedLoader``'s: a run resumes from a ``TokenBatchProducer``
checkpoint and back, at any world size. With ``device="cpu"`` the same code runs with the host
``gather_ragged`` and the host branch of the collate.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _native
from .models.tokens import (META_FIELDS, SharedTokenSource, TokenWindowLayout, collate_token_window,
                            drop_cached_views, ffd_order, in_order_rows)
from .permutation import EpochOrder
from .resident import PrefetchedIndexedLoader
from .types import DDLEnv
from .utils import streams
from .zerocopy import prefault_mapping, register_mapping, unregister_mapping


class ZeroCopyTokenLoader(PrefetchedIndexedLoader):
    def __init__(self, source: SharedTokenSource, global_batch: int, seq_len: int = 4096, mode: str = "pad",
                 env: DDLEnv | None = None, *, seed: int = 0, pack_order: str = "in_order",
                 token_rows: str = "exact", pad_id: int = 0, depth: int = 2, max_blocks: int | None = None,
                 device: str | torch.device | None = None, n_epochs: int | None = None,
                 resume_state: dict | None = None, prefault: bool = True, handoff: str = "host"):
        if handoff not in ("host", "device"):
            raise ValueError("handoff must be 'host' or 'device'")
        if mode not in ("pad", "pack"):
            raise ValueError("mode must be 'pad' or 'pack'")
        if pack_order not in ("in_order", "ffd"):
            raise ValueError("pack_order must be 'in_order' or 'ffd'")
        if pack_order != "in_order" and mode != "pack":
            raise ValueError(f"pack_order={pack_order!r} reorders rows of a PACKED batch; mode={mode!r} has "
                             "one sequence per row")
        if token_rows not in ("exact", "fixed"):
            raise ValueError("token_rows must be 'exact' or 'fixed'")
        self.handoff = handoff  # PCIe-paced batches: no barrier packet in the caller's queue (ZeroCopyLoader)
        self.env = env or DDLEnv()
        self.W, self.rank = self.env.world_size, self.env.rank
        self.source, self.seq_len, self.mode = source, int(seq_len), mode
        self.pack_order, self.token_rows, self.pad_id = pack_order, token_rows, int(pad_id)
        self.order = EpochOrder(source.n, global_batch, seed)
        self.GB, self.LB = int(global_batch), self.order.local_batch(self.W)
        self.out_dtype = torch.int32  # input_ids (the checkpoint's dtype field)
        if max_blocks is None:
            # The image loader's same-width cap of 32 workgroups (ZeroCopyLoader) was the starting point, carried
            # over, not measured for this kernel. This kernel's own sweep says uncapped: where the gather is the
            # limit (2048 sequences per batch) 0 / 32 / 64 workgroups deliver 19.3G / 11.4G / 17.9G tokens/s
            # (profiles/zerocopy_tokens/zerocopy_batch2048.jsonl) -- a tile is one sequence's <= 16 KB hull, 4.4 KB
            # on average, so 32 workgroups hold too few bytes in flight; at 64 sequences per batch the host paces
            # the loader and the cap does not matter (1.99-2.14G, sweep_max_blocks.jsonl)
            max_blocks = 0
        self.max_blocks = int(max_blocks)
        if device is None:
            device = self.env.device or ("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._init_cursor(seed, depth, n_epochs, resume_state)

        lay = self.layout = TokenWindowLayout(self.LB, self.seq_len, source.max_len, 1, source.token_bytes)
        self._reg = lay.regions()
        self._hdr_bytes = self._reg["tokens"][0]  # meta + header arrays: everything in front of the tokens
        # in front of the window: the gather's descriptor, src_start [LB] i64 + tile_start [LB + 1] i32
        self._desc_bytes = -(-(8 * self.LB + 4 * (self.LB + 1)) // 16) * 16
        self._toks = source.tokens.tensor().view(-1)  # keeps the mappings alive
        self._offs_t = source.offsets.tensor().view(-1)
        self._offs = self._offs_t.numpy()
        self.nbytes = int(self._offs[-1]) * source.token_bytes if source.n else 0
        self._reg_base = None
        self.prep_stream = None
        self.prefault_s = 0.0
        gpu = self.device.type == "cuda"
        win_bytes = self._desc_bytes + lay.nbytes
        self._windows = [torch.empty(win_bytes, dtype=torch.uint8, device=self.device) for _ in range(self.depth + 1)]
        if gpu:
            self._reg_base, self._dptr = register_mapping(source.tokens.address, max(self.nbytes, 1), shared=True)
            self.prep_stream = streams.batch_stream(self.device)
            # pinned header slots, one more than the windows: a slot is rewritten only after the copy out of it
            # has completed (its event), which is normally long done
            self._slots = [torch.empty(self._desc_bytes + self._hdr_bytes, dtype=torch.uint8, pin_memory=True)
                           for _ in range(self.depth + 2)]
            self._slot_ev = [None] * len(self._slots)
            if prefault:
                self.prefault_s = prefault_mapping(self._dptr, self.nbytes, self.device, self.prep_stream)
        else:
            self._slots = self._windows  # the CPU twin writes the header straight into the window
        self._views = [self._host_views(b) for b in self._slots]

    def _host_views(self, buf: torch.Tensor) -> dict:
        """numpy views (and raw addresses) of the descriptor and header arrays at the front of a host buffer."""
        a = buf.numpy()
        d, LB = self._desc_bytes, self.LB
        v = {"src_start": a[:8 * LB].view(np.int64), "tile_start": a[8 * LB:8 * LB + 4 * (LB + 1)].view(np.int32)}
        for name in ("meta", "offsets", "row_start", "row_end", "seg_offsets"):
            off, count = self._reg[name]
            v[name] = a[d + off:d + off + 8 * count].view(np.int64)
        v["ptr"] = {k: int(x.ctypes.data) for k, x in v.items()}
        return v

    def _assemble(self, t: int):
        e, g = divmod(t, self.order.batches_per_epoch)
        lay, S, LB, tb = self.layout, self.seq_len, self.LB, self.source.token_bytes
        offs = self._offs
        idx = np.asarray(self.order.indices(e, g, self.rank, self.W), dtype=np.int64)
        lens = offs[idx + 1] - offs[idx]
        pack = self.mode == "pack"
        if pack and self.pack_order == "ffd":
            order, ffd_rows = ffd_order(lens, S)
            if ffd_rows < in_order_rows(lens, S):  # the producer's rule: FFD is kept only if it wins
                idx, lens = idx[order], lens[order]
        gpu = self.prep_stream is not None
        k = t % len(self._slots)
        if gpu and self._slot_ev[k] is not None and not self._slot_ev[k].query():
            self._slot_ev[k].synchronize()  # the H2D copy out of this slot (depth + 2 batches ago)
        v = self._views[k]
        p = v["ptr"]
        v["src_start"][:] = offs[idx]
        v["offsets"][0] = 0
        np.cumsum(lens, out=v["offsets"][1:])
        n_tokens = int(v["offsets"][LB])
        if n_tokens > self._reg["tokens"][1]:
            raise ValueError(f"{n_tokens} tokens exceed the window's {self._reg['tokens'][1]}: the corpus holds a "
                             "sequence longer than source.max_len")
        n_rows = n_seg = max_seg = 0
        if pack:
            cap = lay.max_segments
            n_rows, n_seg = _native.runtime().pack_plan(p["offsets"], LB, S, p["row_start"], p["row_end"], cap,
                                                        p["seg_offsets"], cap)
            if n_seg:
                max_seg = int(np.diff(v["seg_offsets"][: n_seg + 1]).max())
        meta = (n_tokens, n_rows, n_seg, max_seg, 0)
        v["meta"][:META_FIELDS] = meta
        win = self._windows[t % len(self._windows)]
        body = win[self._desc_bytes:]
        tok_off = self._desc_bytes + self._hdr_bytes
        fixed = self.token_rows == "fixed"
        if not gpu:
            _native.runtime().gather_ragged(win.data_ptr() + tok_off, p["offsets"], self._toks.data_ptr(),
                                            self._offs_t.data_ptr(), self.source.n, idx, tb,
                                            self._reg["tokens"][1], 2)
            return collate_token_window(body, lay, self.mode, meta, self.pad_id, fixed_rows=fixed), None
        hip, st = _native.hip(), self.prep_stream
        n_tiles = hip.ragged_tile_plan(self._dptr, p["src_start"], p["offsets"], LB, tb, p["tile_start"])
        with streams.on_stream(st):
            w = win.data_ptr()
            hip.memcpy_h2d(w, self._slots[k].data_ptr(), tok_off, st.cuda_stream)
            if self._slot_ev[k] is None:
                self._slot_ev[k] = torch.cuda.Event()
            self._slot_ev[k].record(st)
            hip.gather_ragged(dst=w + tok_off, src=self._dptr, src_start=w,
                              dst_offsets=w + self._desc_bytes + self._reg["offsets"][0], tile_start=w + 8 * LB,
                              n=LB, n_tiles=n_tiles, elem_bytes=tb, max_blocks=self.max_blocks, stream=st.cuda_stream)
            batch = collate_token_window(body, lay, self.mode, meta, self.pad_id, fixed_rows=fixed)
            ev = torch.cuda.Event()
            ev.record(st)
        return batch, ev

    def stats(self) -> dict:
        return {"batches": self.batches, "source_bytes": self.nbytes, "max_blocks": self.max_blocks,
                "handoff": self.handoff, "host_waits": self.host_waits, "prefault_s": self.prefault_s}

    def close(self) -> None:
        if self.prep_stream is not None:
            self.prep_stream.synchronize()
        self._queue.clear()
        if self._windows:
            drop_cached_views(w.data_ptr() + self._desc_bytes for w in self._windows)
            self._windows = []
        if self._reg_base is not None:
            unregister_mapping(self._reg_base, self.device, shared=True)  # synchronises before unregistering
            self._reg_base = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass
