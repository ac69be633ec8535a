"""The corpus replica in HBM, and what the loaders that read it have in common.

``CorpusReplica`` is one tokenised corpus copied into one HBM allocation, shared by every loader over that corpus
on that device (train + eval; the sequence-batched and the stream format) and freed when the last one closes.
``ResidentCorpusLoader`` is mixed into those loaders (``ResidentTokenLoader``, ``ResidentTokenStreamLoader``) in
front of their ``PrefetchedIndexedLoader`` base: it attaches and releases the replica, caches the ``RowIndex``
selectors of an epoch, frames a step's launches on the prep stream and keeps the two timings the benchmark reads.
"""

from __future__ import annotations

import time

import torch

from . import _native
from .exceptions import DDLError
from .ops.kernels import row_selector
from .utils import streams
from .zerocopy import register_mapping, unregister_mapping

REPLICAS: dict[tuple, "CorpusReplica"] = {}  # (corpus address, bytes, device index) -> the replica


class CorpusReplica:
    def __init__(self, key: tuple, hbm: torch.Tensor, load_s: float):
        self.key, self.hbm, self.load_s = key, hbm, load_s
        self.users = 1
        self.offsets_dev = None  # the corpus offsets in HBM, once a loader has asked (offsets)

    @classmethod
    def acquire(cls, source, nbytes: int, device: torch.device, stream, hbm_fraction: float,
                chunk_bytes: int) -> tuple["CorpusReplica", bool]:
        """(the corpus in HBM, shared with an earlier loader). A new replica is budgeted against the free HBM
        first; a failure leaves nothing allocated or registered."""
        key = (int(source.tokens.address), int(nbytes), device.index)
        rep = REPLICAS.get(key)
        if rep is not None:
            rep.users += 1
            return rep, True
        free, _ = torch.cuda.mem_get_info(device)
        if nbytes > hbm_fraction * free:
            raise DDLError(f"the corpus ({nbytes} bytes) exceeds hbm_fraction={hbm_fraction} of the free HBM "
                           f"({free} bytes free, {int(hbm_fraction * free)} allowed); a corpus is not sharded across "
                           "ranks: use ZeroCopyTokenLoader (batches of sequences) or ZeroCopyTokenStreamLoader (the "
                           "stream format), which read it from host memory")
        t0 = time.perf_counter()
        hip = _native.hip()
        hbm = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        if nbytes:
            torch.cuda.synchronize(device)  # the block may be a cached one: nothing of its past is still running
            base, _ = register_mapping(source.tokens.address, nbytes, shared=True)  # pinned: the copies are SDMA
            try:
                step = max(1, int(chunk_bytes))
                for o in range(0, nbytes, step):
                    hip.memcpy_h2d(hbm.data_ptr() + o, source.tokens.address + o, min(step, nbytes - o),
                                   stream.cuda_stream)
                stream.synchronize()
            finally:
                unregister_mapping(base, device, shared=True)
        rep = REPLICAS[key] = cls(key, hbm, time.perf_counter() - t0)
        return rep, False

    def offsets(self, offsets_t: torch.Tensor, stream) -> torch.Tensor:
        """The corpus offsets (int64 [n + 1]) in HBM, for plans built on the device: uploaded once per replica by
        the first loader that asks, shared and freed with it."""
        if self.offsets_dev is None:
            with streams.on_stream(stream):
                self.offsets_dev = offsets_t.to(self.hbm.device)
            stream.synchronize()  # bring-up: later loaders over this replica use it from their own streams
        return self.offsets_dev

    def release(self) -> None:
        """One holder less (a holder releases once: ``ResidentCorpusLoader._release_replica`` forgets it)."""
        if REPLICAS.get(self.key) is not self:
            return
        self.users -= 1
        if self.users <= 0:
            del REPLICAS[self.key]  # the last reference: the allocation goes back to the allocator


class ResidentCorpusLoader:
    """Mixed in before ``PrefetchedIndexedLoader``. The loader gives ``_step(t) -> (batch, ready event)`` and
    ``_perm(epoch)``; it has ``source``, ``nbytes``, ``device``, ``prep_stream`` and ``_windows`` of its own."""

    _replica = None

    def _init_frame(self) -> None:
        """The fields of the launch frame and its timings (a loader that reads the corpus where it lies, such as
        ``ZeroCopyTokenStreamLoader``, uses the frame without a replica)."""
        self.assemble_s = 0.0  # wall time spent in _assemble (host_us_per_step of the benchmark)
        self.profile_every = 0  # > 0: device events around the launches of every profile_every-th step
        self._kernel_evs: list = []
        self._selectors: dict = {}

    def _attach_replica(self, hbm_fraction: float, chunk_bytes: int) -> bool:
        """The fields every resident loader reports, and on the GPU the replica. True on the GPU."""
        self.replica_shared = False
        self.load_s = 0.0
        self._init_frame()
        if self.prep_stream is None:
            return False
        self._replica, self.replica_shared = CorpusReplica.acquire(
            self.source, self.nbytes, self.device, self.prep_stream, float(hbm_fraction), chunk_bytes)
        self.load_s = self._replica.load_s
        return True

    def _release_replica(self) -> None:
        rep, self._replica = self._replica, None
        if rep is not None:
            rep.release()

    @property
    def replica_ptr(self) -> int | None:
        """Device address of the corpus replica (None on the CPU, and after ``close``)."""
        rep = self._replica
        return rep.hbm.data_ptr() if rep is not None else None

    def _selector(self, epoch: int, perm_of=None) -> dict:
        """The ``RowIndex`` arguments (``ops.row_selector``) of ``perm_of(epoch)``, by default the epoch's order
        ``_perm(epoch)`` -- a permutation's Feistel round keys, the identity for None -- at base 0: a step that
        starts elsewhere passes ``dict(sel, base=...)``."""
        sel = self._selectors.get((epoch, perm_of))
        if sel is None:
            if len(self._selectors) > 8:
                self._selectors.clear()
            sel = self._selectors[epoch, perm_of] = row_selector(None, (perm_of or self._perm)(epoch), 0)
        return sel

    def _assemble(self, t: int):
        t_host = time.perf_counter()
        out = self._step(t)
        self.assemble_s += time.perf_counter() - t_host
        return out

    def _launch(self, t: int, nbytes: int, issue):
        """The frame of a GPU step, on the prep stream: ``issue(window, whole)`` puts the step's launches there,
        given the step's plan window and ``whole``, one allocation of ``nbytes`` for everything the caller may
        hold (a held batch survives the ring of windows); every ``profile_every``-th step they run between two
        timing events. Returns (what ``issue`` returned, the batch's ready event)."""
        st = self.prep_stream
        timed = self.profile_every > 0 and t % self.profile_every == 0
        win = self._windows[t % len(self._windows)]
        with streams.on_stream(st):
            whole = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if timed:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(st)
            r = issue(win, whole)
            if timed:
                ev1.record(st)
                self._kernel_evs.append((ev0, ev1))
            ev = torch.cuda.Event()
            ev.record(st)
        return r, ev

    def timing(self) -> dict:
        """``host_us_per_step``: mean wall time of ``_assemble`` (planning, copies and launches, on the host);
        ``kernel_us``: mean device time of the sampled steps' launches (``profile_every``), None without samples.
        Synchronises the prep stream."""
        steps = max(1, self.batches + len(self._queue))  # batches assembled so far
        out = {"host_us_per_step": 1e6 * self.assemble_s / steps, "kernel_us": None,
               "kernel_samples": len(self._kernel_evs)}
        if self._kernel_evs:
            self.prep_stream.synchronize()
            out["kernel_us"] = 1e3 * sum(a.elapsed_time(b) for a, b in self._kernel_evs) / len(self._kernel_evs)
        return out
