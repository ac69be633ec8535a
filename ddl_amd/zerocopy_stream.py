"""Producer-free zero-copy token stream loader: the stream format of ``ResidentTokenStreamLoader`` -- every step
``B`` rows of exactly ``S`` tokens cut from the concatenation of the epoch's shuffled documents -- out of a corpus
that stays in host memory.

``ResidentTokenStreamLoader`` needs the whole corpus in HBM and refuses one that does not fit next to the model.
Its table and plan kernels never read a token, though: they read the corpus offsets (8 bytes per document) and the
Feistel keys. Here only the offsets are uploaded; the tokens (node shm) are registered once, page-rounded, as
pinned, device-mapped memory (shared with any other zero-copy loader over the corpus), and per step the prep stream
runs

* ``token_stream_plan`` (or ``token_stream_plan_rows`` with ``shuffle_rows``), exactly as the resident loader;
* ``gather_stream_pieces``: the plan's pieces, read over PCIe in 16-byte aligned non-temporal loads of their
  aligned hulls, into a staging window of ``LB * S`` ids in HBM -- every token of the batch crosses the link once,
  nothing else does, and the grid is capped by ``max_blocks``;
* the unchanged ``pad_pack_tokens_indexed`` with the staging window as its corpus.

Nothing is planned on the host, nothing is copied, no host read of device memory, no synchronisation per step or
per epoch. The epoch, table, selector and checkpoint logic is ``token_stream.TokenStreamLoader``'s, shared with the
resident loader: the batches are the same key by key (``shuffle_rows``, ``mix`` and ``labels`` included) and the
same at every world size, and a run resumes from a resident stream checkpoint (``kind="token_stream"``) and back.
With ``device="cpu"`` the loader runs the definition, ``ops.ref_stream_tokens``.

HBM use does not scale with the corpus's tokens: ``stats()["hbm_bytes"]`` is

    8 * (2 * (n_order + 1) + token_stream_table_scratch(n_order) + (2 * n_order with a mix))      tables, orders
    + 8 * (n_documents + 1)                                                                        offsets
    + (depth + 1) * ops.stream_zerocopy_window_bytes(LB, S, max_segments, token_bytes, shuffle_rows)   windows
                                                                      (+ 4 * LB * S each with ``fim``, 16-byte aligned)

(the batches a caller holds are its own). The corpus must fit in host memory.
"""

from __future__ import annotations

import torch

from .exceptions import DDLError
from .models.tokens import SharedTokenSource
from .ops.kernels import launch_stream_plan_rows_zerocopy, launch_stream_plan_zerocopy, stream_zerocopy_window_bytes
from .token_fim import TokenFIM
from .token_mix import TokenMix
from .token_stream import TokenStreamLoader
from .types import DDLEnv
from .utils import streams
from .zerocopy import prefault_mapping, register_mapping, unregister_mapping


class ZeroCopyTokenStreamLoader(TokenStreamLoader):
    _launch_plan = staticmethod(launch_stream_plan_zerocopy)
    _launch_plan_rows = staticmethod(launch_stream_plan_rows_zerocopy)

    def __init__(self, source: SharedTokenSource, global_batch: int, seq_len: int = 4096, env: DDLEnv | None = None,
                 *, seed: int = 0, shuffle: bool = True, pad_id: int = 0, depth: int = 2,
                 max_blocks: int | None = None, device: str | torch.device | None = None,
                 n_epochs: int | None = None, resume_state: dict | None = None, prefault: bool = True,
                 handoff: str = "host", chunk_bytes: int = 256 << 20, max_segments: int | None = None,
                 labels: bool = False, ignore_index: int = -100, shuffle_rows: bool = False,
                 mix: TokenMix | None = None, fim: TokenFIM | None = None):
        """``ResidentTokenStreamLoader``'s arguments without ``hbm_fraction`` (no token is kept in HBM;
        ``chunk_bytes`` is accepted and unused, so that a call site can switch loaders), with ``max_blocks`` (the
        cap of the gather's grid, 0: none) and ``prefault`` (touch every page of the mapping once before the first
        batch) of ``ZeroCopyTokenLoader``. ``handoff`` defaults to "host": PCIe-paced batches, no barrier packet
        in the caller's queue."""
        self._reg_base = None
        self.prefault_s = 0.0
        self._init_stream(source, global_batch, seq_len, env, seed=seed, shuffle=shuffle, pad_id=pad_id, depth=depth,
                          device=device, n_epochs=n_epochs, resume_state=resume_state, handoff=handoff,
                          max_segments=max_segments, labels=labels, ignore_index=ignore_index,
                          shuffle_rows=shuffle_rows, mix=mix, fim=fim)
        if max_blocks is None:
            # swept once (profiles/zerocopy_stream/sweep_max_blocks.jsonl): 0 / 32 / 64 workgroups deliver
            # 2.61-2.81G / 2.12G / 2.63G tokens/s at 64 rows per step and 15.85-16.22G / 13.36G / 15.55G at 2048 --
            # a chunk is 16 KB of the window, so a capped grid holds too few bytes in flight: uncapped
            max_blocks = 0
        self.max_blocks = int(max_blocks)
        if self.max_blocks < 0:
            raise ValueError("max_blocks must be >= 0")
        self._init_frame()
        if self.prep_stream is None:
            return
        try:
            need = self.hbm_bytes
            free, _ = torch.cuda.mem_get_info(self.device)
            if need > free:
                raise DDLError(f"the tables, offsets and windows ({need} bytes) exceed the free HBM ({free} bytes)")
            self._reg_base, self._corpus_ptr = register_mapping(source.tokens.address, max(self.nbytes, 1),
                                                                shared=True)
            with streams.on_stream(self.prep_stream):
                self._offsets_dev = self._offs_t.to(self.device)
            self._init_tables()
            self.prep_stream.synchronize()  # bring-up: the pageable offsets are on the device
            if prefault:
                self.prefault_s = prefault_mapping(self._corpus_ptr, self.nbytes, self.device, self.prep_stream)
        except Exception:
            self.close()
            raise

    def _launch_kw(self) -> dict:
        return {"max_blocks": self.max_blocks}

    def _window_bytes(self) -> int:
        return stream_zerocopy_window_bytes(self.LB, self.seq_len, self.max_segments, self.source.token_bytes,
                                            self.shuffle_rows) + self._fim_bytes

    @property
    def hbm_bytes(self) -> int:
        """Device memory the loader itself holds (the module's text has the sum): independent of the tokens."""
        if self.device.type != "cuda":
            return 0
        return (self._table_bytes() + 8 * (self.n_documents + 1)
                + (self.depth + 1) * self._window_bytes())

    def stats(self) -> dict:
        return {"batches": self.batches, "source_bytes": self.nbytes, "max_blocks": self.max_blocks,
                "handoff": self.handoff, "host_waits": self.host_waits, "prefault_s": self.prefault_s,
                "format": "stream", "hbm_bytes": self.hbm_bytes, "rows_per_epoch": self.order.n_samples,
                "max_segments": self.max_segments, "tables_built": self.tables_built,
                "shuffle_rows": self.shuffle_rows, "mix_parts": self.mix.parts if self.mix is not None else 0,
                "mix_documents": self.n_order, "orders_built": self.orders_built, "fim": self.fim is not None}

    def close(self) -> None:
        self._close_stream()
        self._offsets_dev = None
        base, self._reg_base = getattr(self, "_reg_base", None), None
        if base is not None:
            unregister_mapping(base, self.device, shared=True)  # synchronises before unregistering
