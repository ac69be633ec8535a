"""HBM-resident token loader (BASELINE config 4): the corpus is copied into HBM once, and every batch is packed
straight out of it by one kernel.

``TokenBatchProducer`` and ``ZeroCopyTokenLoader`` put the PCIe link and host DRAM under every token of every
epoch. A tokenised corpus is the dataset most likely to fit in HBM (2 bytes per id: 10B tokens are 20 GB of
288), and once it is there a step needs no link, no host DRAM pass and no producers, so a rank's rate no longer
depends on how many ranks share a socket. Here

* bring-up copies the corpus tokens (node shm) into one HBM allocation in ``chunk_bytes`` pieces: the mapping is
  registered (shared with any zero-copy loader over it), copied with SDMA and unregistered again. The offsets
  stay on the host, where the plan is built. At W > 1 every rank loads its own full replica, with no
  collective; a corpus larger than ``hbm_fraction`` of the free HBM is refused (sharding is not supported: use
  ``ZeroCopyTokenLoader``, or ``ZeroCopyTokenStreamLoader`` for the stream format). Loaders over one corpus on
  one device (train + eval) share one replica, counted per process and freed when the last one closes;
* per step the host does what ``ZeroCopyTokenLoader`` does minus the tile plan: this rank's ``EpochOrder``
  indices, the lengths, the producer's FFD rule, the native ``pack_plan`` -- written as a
  ``TokenWindowLayout(k=1)`` header plus ``src_start`` / ``seg_src`` into a slot of a small pinned ring;
* the prep stream copies that slot to the device (one small H2D) and launches ``pad_pack_tokens_indexed`` once:
  it writes the model inputs of the virtual stream ``concat(corpus[src_start[i] : src_start[i] + len_i])``
  reading every token from the corpus -- no flat window is written and read back.

The batches are those of the other two token paths, key by key, and the order and the ``kind="indexed"``
checkpoint are ``PrefetchedIndexedLoader``'s: a run resumes from a ``TokenBatchProducer`` or
``ZeroCopyTokenLoader`` checkpoint and back, at any world size. With ``device="cpu"`` the same planning runs
with the host ``gather_ragged`` and the host collate.

``plan="device"`` (in-order packing only) moves that host work to the device: the corpus offsets are uploaded
next to the replica, and per step the host computes the batch's base position in the epoch order, fetches the
epoch's Feistel round keys and issues launches -- ``token_batch_descriptor`` (index, lengths, running offsets,
each segment's corpus element), ``pack_plan_device`` and ``pad_pack_tokens_indexed`` reading the plan's counts
from device memory. No NumPy, no pinned slot, no H2D copy, no host read of anything the device wrote; the shapes
are therefore static and the counts of a batch are 0-d device tensors (``docs/ARCHITECTURE.md``).

``plan="device", mode="pack", pack_order="ffd_device"`` adds the producer's FFD rule to that path without bringing
the host back: one more launch, ``token_ffd_order`` (one workgroup: lengths, a sort and a first-fit placement in
LDS), writes the batch's corpus indices in first-fit-decreasing order when that needs fewer rows, and the three
launches run on that index. The batches are those of ``plan="host", pack_order="ffd", token_rows="fixed"``, at most
``ops.FFD_MAX_SEQS`` sequences per rank and step. ``max_rows`` (device pack plan only) makes every batch that many
rows instead of the worst case ``layout.max_segments``, so the denser plan reaches the model as a smaller static
shape; a batch that needs more comes back as padding with ``n_rows = -1`` (the plan kernel's overflow contract).
"""

from __future__ import annotations

import numpy as np
import torch

from . import _native
from .corpus_replica import ResidentCorpusLoader
from .models.tokens import SharedTokenSource, check_token_options, drop_cached_views
from .ops.kernels import (carve_token_outputs, check_ffd_count, device_batch_bytes, device_plan_bytes,
                          launch_device_plan,
                          pack_tokens_indexed_device, pad_tokens_indexed_device, segment_sources,
                          token_output_bytes)
from .token_plan import HostPlannedTokenLoader
from .types import DDLEnv
from .utils import streams


class ResidentTokenLoader(ResidentCorpusLoader, HostPlannedTokenLoader):
    def __init__(self, source: SharedTokenSource, global_batch: int, seq_len: int = 4096, mode: str = "pad",
                 env: DDLEnv | None = None, *, seed: int = 0, pack_order: str = "in_order",
                 token_rows: str | None = None, pad_id: int = 0, depth: int = 2,
                 device: str | torch.device | None = None, n_epochs: int | None = None,
                 resume_state: dict | None = None, handoff: str = "device", hbm_fraction: float = 0.8,
                 chunk_bytes: int = 256 << 20, plan: str = "host", labels: bool = False, ignore_index: int = -100,
                 max_rows: int | None = None):
        if plan not in ("host", "device"):
            raise ValueError("plan must be 'host' or 'device'")
        ffd_device = pack_order == "ffd_device"
        if ffd_device:
            if plan != "device" or mode != "pack":
                raise ValueError("pack_order='ffd_device' is the first-fit-decreasing order built by a kernel: it "
                                 "needs plan='device', mode='pack' (with plan='host' use pack_order='ffd')")
            pack_order = "in_order"  # what the shared checks and the host-side planner know
            check_ffd_count(int(global_batch) // (env or DDLEnv()).world_size)  # the batch of one rank
        if max_rows is not None and (plan != "device" or mode != "pack" or int(max_rows) < 1):
            raise ValueError("max_rows (>= 1) is the static row count of plan='device', mode='pack' batches; the "
                             "other paths size their batches themselves")
        if token_rows is None:  # unset: the host plan sizes every batch exactly, the device plan cannot
            token_rows = "fixed" if plan == "device" and mode == "pack" else "exact"
        check_token_options(mode, pack_order, token_rows, handoff)
        if plan == "device":
            if pack_order == "ffd":
                raise ValueError("pack_order='ffd' is a sequential bin packing that plan='device' does not build: "
                                 "use plan='host' (the host plan) for first-fit-decreasing rows")
            if mode == "pack" and token_rows != "fixed":
                raise ValueError("plan='device' packs into static shapes (the host never learns the row count): "
                                 "token_rows must be 'fixed'; token_rows='exact' needs plan='host'")
        self.plan = plan
        # handoff "device": batches take microseconds, not a PCIe transfer: the caller's stream waits
        super().__init__(source, global_batch, seq_len, mode, env, seed=seed, pack_order=pack_order,
                         token_rows=token_rows, pad_id=pad_id, depth=depth, device=device, n_epochs=n_epochs,
                         resume_state=resume_state, handoff=handoff, labels=labels, ignore_index=ignore_index)
        lay = self.layout
        self.max_rows = None if max_rows is None else int(max_rows)
        self._rows = lay.max_segments if max_rows is None else int(max_rows)  # the device pack plan's static rows
        self._ffd = ffd_device
        if ffd_device:
            self.pack_order = "ffd_device"
        if plan == "device" and self.LB * source.max_len > 0x7FFFFFFF:  # the host plan checks every batch instead
            raise ValueError(f"{self.LB} sequences of up to {source.max_len} tokens in one batch can overflow int32 "
                             "cu_seqlens")
        self.n_elems = self.nbytes // source.token_bytes
        gpu = self._attach_replica(hbm_fraction, chunk_bytes)
        if plan == "device":
            self._init_device_plan(gpu)
            return
        # on the GPU a window is descriptor + header only: no token ever lands there
        self._init_ring(self._desc_bytes + (self._hdr_bytes if gpu else lay.nbytes))

    def _desc_extra(self) -> tuple:
        return "seg_src", np.int64, self.layout.max_segments  # the corpus element of each segment's first token

    def _init_device_plan(self, gpu: bool) -> None:
        """plan="device": the corpus offsets in HBM and a ring of plan windows (the arrays between the launches;
        nothing a caller holds). The CPU twin needs neither."""
        lay, pack = self.layout, self.mode == "pack"
        self._max_seqlen = min(self.seq_len, self.source.max_len)
        if not gpu:
            return
        self._replica.offsets(self._offs_t, self.prep_stream)
        segs = lay.max_segments if pack else None
        self._plan_bytes = device_plan_bytes(self.LB, segs, self._rows if pack else 0, ffd=self._ffd)
        self._batch_bytes = device_batch_bytes(self._rows if pack else self.LB, self.seq_len, segs,
                                               labels=self.labels)
        self._windows = [torch.empty(self._plan_bytes, dtype=torch.uint8, device=self.device)
                         for _ in range(self.depth + 1)]

    def _perm(self, epoch: int):
        return self.order.perm(epoch) if self.order.shuffle else None

    def _step_device_plan(self, t: int):
        e, g = divmod(t, self.order.batches_per_epoch)
        base = g * self.GB + self.rank * self.LB
        lay, S, LB, pack = self.layout, self.seq_len, self.LB, self.mode == "pack"
        if self.prep_stream is None:  # the CPU twin: the op's reference path
            kw = dict(perm=self._perm(e), base=base, count=LB, seq_len=S, pad_id=self.pad_id, labels=self.labels,
                      ignore_index=self.ignore_index)
            if pack:
                r = pack_tokens_indexed_device(self._toks, self._offs_t, max_rows=self._rows,
                                               max_segs=lay.max_segments,
                                               pack_order="ffd" if self._ffd else "in_order", **kw)
            else:
                r = pad_tokens_indexed_device(self._toks, self._offs_t, **kw)
            ev = None
        else:
            rep = self._replica
            r, ev = self._launch(t, self._batch_bytes, lambda win, whole: launch_device_plan(
                win.data_ptr(), whole, corpus_ptr=rep.hbm.data_ptr(), corpus_elems=self.n_elems,
                tok16=self.source.token_bytes == 2, corpus_offsets_ptr=rep.offsets_dev.data_ptr(),
                n_corpus=self.source.n, selector=dict(self._selector(e), base=base), n=LB, seq_len=S,
                pad_id=self.pad_id, pack=pack, max_segs=lay.max_segments if pack else 0,
                max_rows=self._rows if pack else 0, stream=self.prep_stream.cuda_stream, labels=self.labels,
                ignore_index=self.ignore_index, ffd=self._ffd))
        counts = r.pop("counts")
        r["n_tokens"] = counts[2]
        if pack:
            r["max_seqlen"] = self._max_seqlen  # a static upper bound (varlen attention accepts one)
            r["n_rows"], r["n_seg"] = counts[0], counts[1]
        return r, ev

    def _step(self, t: int):
        if self.plan == "device":
            return self._step_device_plan(t)
        k, v, idx, meta = self._plan(t)
        n_tokens, n_rows, n_seg, max_seg, _ = meta
        if self.prep_stream is None:
            return self._cpu_batch(t, v, idx, meta), None
        if n_tokens > 0x7FFFFFFF:
            raise ValueError(f"{n_tokens} tokens in one batch overflow int32 cu_seqlens")
        lay, S, LB = self.layout, self.seq_len, self.LB
        pack, fixed = self.mode == "pack", self.token_rows == "fixed"
        if pack and n_seg:
            v["seg_src"][:n_seg] = segment_sources(v["src_start"], v["offsets"], v["seg_offsets"], n_seg)
        hip, st = _native.hip(), self.prep_stream
        fill = lay.max_segments if (pack and fixed) else 0
        R = max(n_rows, fill) if pack else LB
        # the frame of ResidentCorpusLoader._launch, written out: this step has an H2D copy and the carving in
        # front of the timed launch, and the calls _launch makes cost it 1.5-3 us of its 37 (pad mode)
        timed = self.profile_every > 0 and t % self.profile_every == 0
        win = self._windows[t % len(self._windows)]
        with streams.on_stream(st):
            w = win.data_ptr()
            self._upload(hip, k, win)
            # one allocation for all outputs (ops.carve_token_outputs): memory of its own, so a held batch
            # survives the rings
            whole = torch.empty(token_output_bytes(R, S, n_seg if pack else None, labels=self.labels),
                                dtype=torch.uint8, device=self.device)
            ids, mask, pos, seg, cu, *lab = carve_token_outputs(whole, R, S, n_seg if pack else None,
                                                                labels=self.labels)
            h = w + self._desc_bytes
            if timed:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(st)
            hip.pad_pack_tokens_indexed(
                corpus=self._replica.hbm.data_ptr(), corpus_elems=self.n_elems, src_start=w, seg_src=w + 8 * LB,
                offsets=h + self._reg["offsets"][0], row_start=h + self._reg["row_start"][0],
                row_end=h + self._reg["row_end"][0], seg_offsets=h + self._reg["seg_offsets"][0], n_seg=n_seg,
                out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(), pos_is_i64=True,
                segment_ids=seg.data_ptr() if pack else 0, cu_seqlens_out=cu.data_ptr() if pack else 0,
                rows=n_rows if pack else LB, seq_len=S, pad_id=self.pad_id, mode=1 if pack else 0,
                stream=st.cuda_stream, fill_rows=fill, tok16=self.source.token_bytes == 2,
                labels=lab[0].data_ptr() if lab else 0, ignore_index=self.ignore_index)
            if timed:
                ev1.record(st)
                self._kernel_evs.append((ev0, ev1))
            ev = torch.cuda.Event()
            ev.record(st)
        if pack:
            batch = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "segment_ids": seg,
                     "cu_seqlens": cu, "max_seqlen": max_seg, "n_tokens": n_tokens}
            if fixed:
                batch["n_rows"] = n_rows
        else:
            batch = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "n_tokens": n_tokens}
        if lab:
            batch["labels"] = lab[0]
        return batch, ev

    def stats(self) -> dict:
        out = {"batches": self.batches, "source_bytes": self.nbytes, "load_s": self.load_s,
               "load_gbps": self.nbytes / self.load_s / 1e9 if self.load_s > 0 else 0.0,
               "handoff": self.handoff, "host_waits": self.host_waits, "replica_shared": self.replica_shared}
        if self.plan != "host":  # the default mode's stats stay exactly as they were
            out["plan"] = self.plan
        if self._ffd:
            out["pack_order"] = self.pack_order
        return out

    def close(self) -> None:
        if self.prep_stream is not None:
            self.prep_stream.synchronize()
        self._queue.clear()
        self._kernel_evs = []
        if self._windows:
            if self.prep_stream is None and self.plan == "host":
                drop_cached_views(w.data_ptr() + self._desc_bytes for w in self._windows)
            self._windows = []
        self._release_replica()
