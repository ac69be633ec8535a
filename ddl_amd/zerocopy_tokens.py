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
from .models.tokens import SharedTokenSource, check_token_options, collate_token_window, drop_cached_views
from .token_plan import HostPlannedTokenLoader
from .types import DDLEnv
from .utils import streams
from .zerocopy import prefault_mapping, register_mapping, unregister_mapping


class ZeroCopyTokenLoader(HostPlannedTokenLoader):
    def __init__(self, source: SharedTokenSource, global_batch: int, seq_len: int = 4096, mode: str = "pad",
                 env: DDLEnv | None = None, *, seed: int = 0, pack_order: str = "in_order",
                 token_rows: str = "exact", pad_id: int = 0, depth: int = 2, max_blocks: int | None = None,
                 device: str | torch.device | None = None, n_epochs: int | None = None,
                 resume_state: dict | None = None, prefault: bool = True, handoff: str = "host",
                 labels: bool = False, ignore_index: int = -100):
        check_token_options(mode, pack_order, token_rows, handoff)
        # handoff "host": PCIe-paced batches, no barrier packet in the caller's queue (ZeroCopyLoader)
        super().__init__(source, global_batch, seq_len, mode, env, seed=seed, pack_order=pack_order,
                         token_rows=token_rows, pad_id=pad_id, depth=depth, device=device, n_epochs=n_epochs,
                         resume_state=resume_state, handoff=handoff, labels=labels, ignore_index=ignore_index)
        if max_blocks is None:
            # The image loader's same-width cap of 32 workgroups (ZeroCopyLoader) was the starting point, carried
            # over, not measured for this kernel. This kernel's own sweep says uncapped: where the gather is the
            # limit (2048 sequences per batch) 0 / 32 / 64 workgroups deliver 19.3G / 11.4G / 17.9G tokens/s
            # (profiles/zerocopy_tokens/zerocopy_batch2048.jsonl) -- a tile is one sequence's <= 16 KB hull, 4.4 KB
            # on average, so 32 workgroups hold too few bytes in flight; at 64 sequences per batch the host paces
            # the loader and the cap does not matter (1.99-2.14G, sweep_max_blocks.jsonl)
            max_blocks = 0
        self.max_blocks = int(max_blocks)
        self._reg_base = None
        self.prefault_s = 0.0
        self._init_ring(self._desc_bytes + self.layout.nbytes)  # the window holds the gathered tokens too
        if self.prep_stream is not None:
            self._reg_base, self._dptr = register_mapping(source.tokens.address, max(self.nbytes, 1), shared=True)
            if prefault:
                self.prefault_s = prefault_mapping(self._dptr, self.nbytes, self.device, self.prep_stream)

    def _desc_extra(self) -> tuple:
        return "tile_start", np.int32, self.LB + 1  # the gather's tile map

    def _assemble(self, t: int):
        k, v, idx, meta = self._plan(t)
        if self.prep_stream is None:
            return self._cpu_batch(t, v, idx, meta), None
        p, LB, tb = v["ptr"], self.LB, self.source.token_bytes
        win = self._windows[t % len(self._windows)]
        tok_off = self._desc_bytes + self._hdr_bytes
        hip, st = _native.hip(), self.prep_stream
        n_tiles = hip.ragged_tile_plan(self._dptr, p["src_start"], p["offsets"], LB, tb, p["tile_start"])
        with streams.on_stream(st):
            w = win.data_ptr()
            self._upload(hip, k, win)
            hip.gather_ragged(dst=w + tok_off, src=self._dptr, src_start=w,
                              dst_offsets=w + self._desc_bytes + self._reg["offsets"][0], tile_start=w + 8 * LB,
                              n=LB, n_tiles=n_tiles, elem_bytes=tb, max_blocks=self.max_blocks, stream=st.cuda_stream)
            batch = collate_token_window(win[self._desc_bytes:], self.layout, self.mode, meta, self.pad_id,
                                         fixed_rows=self.token_rows == "fixed", labels=self.labels,
                                         ignore_index=self.ignore_index)
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
