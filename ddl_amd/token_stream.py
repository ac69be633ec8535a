"""HBM-resident token stream loader: every step is ``B`` rows of exactly ``S`` tokens, cut from the
concatenation of the epoch's shuffled documents (the GPT pre-training format of Megatron's GPT dataset and
nanoGPT).

The sequence-batched token paths deliver ``LB`` documents per step, padded or packed into however many rows
they need; in-order packing fills about 75% of the row space. Here the epoch's token stream is

    stream_e = concat(document perm_e(0), perm_e(1), ..., perm_e(n - 1))        (no separator: documents carry
                                                                                  their own EOS)

and row ``r`` of the epoch is ``stream_e[r * S : (r + 1) * S]``: 100% dense, static-shaped, and the same rows at
every world size (rank ``r`` of ``W`` takes rows ``[g * GB + r * LB, g * GB + (r + 1) * LB)`` of global batch
``g``). ``rows_per_epoch = T // S`` and ``batches_per_epoch = rows_per_epoch // global_batch``; the tail is
dropped, a different one each epoch under ``shuffle``.

Nothing is planned on the host. The corpus replica and its offsets are a ``CorpusReplica`` (shared with
any ``ResidentTokenLoader`` over the same corpus). Once per epoch the ``token_stream_table`` kernels scan the
documents' lengths in the
epoch's order (the Feistel permutation inline) into ``table [n + 1]``; per step ``token_stream_plan`` finds the
window's documents in it and writes the pack plan -- a segment is a maximal run of one document inside one row,
``position_ids`` restart in every segment -- which the unchanged ``pad_pack_tokens_indexed`` renders: two
launches, no copy, no host read of device memory, no synchronisation per step or per epoch (two tables are
kept, since prefetch crosses the epoch boundary; everything is ordered by the prep stream). ``ops.ref_stream_tokens``
is the definition; with ``device="cpu"`` the loader runs it and gives the same dict.

``TokenStreamLoader`` holds everything of this that does not depend on where the tokens lie; for a corpus that does
not fit in HBM ``zerocopy_stream.ZeroCopyTokenStreamLoader`` delivers the same batches out of pinned host memory.

``shuffle_rows=True`` adds the sample shuffle of the format (Megatron's ``shuffle_idx``): in stream order every
document longer than ``S`` puts all its pieces into neighbouring rows of one step. Global batch ``g`` of epoch
``e`` is then rows ``rho_e(g * GB + j)``, ``j < GB`` (rank ``r`` takes ``j`` in ``[r * LB, (r + 1) * LB)``), with
``rho_e = FeistelPermutation(rows_per_epoch, row_seed, e)`` and ``row_seed = permutation.row_seed_for(seed)``; the
rows dropped at the epoch's end are a different set each epoch. The batches stay dense, static-shaped and the
same at every world size. ``token_stream_plan_rows`` (two launches, one wave per row) takes the place of
``token_stream_plan``, the emit launch is the same: three launches per step, and two more cached selectors per
epoch on the host.

``mix=TokenMix(bounds, repeat)`` weights parts of the corpus by document order: the epoch's order is then
``ops.ref_mix_order`` -- ``N'`` entries, a document of part ``p`` appearing ``floor(repeat[p])`` or one more times --
instead of a permutation of the corpus, and everything above holds with ``order_e[i]`` in the place of
``perm_e(i)``. Two neighbouring copies of a document are two segments. Once per epoch ``token_mix_order`` writes the
order into one of two int64 buffers of ``N'`` entries (next to the two tables, on the prep stream, in front of the
table scan), and the table, plan and emit kernels read it as an explicit index: still no copy, no host read of
device memory and no synchronisation. The extra documents of a fractional repeat are the same in every epoch
(``token_mix``), which keeps ``total_tokens``, the rows and batches per epoch and the checkpoint cursor constant.

``fim=TokenFIM(rate, ...)`` rearranges a share of every batch's segments for fill-in-the-middle training
(``token_fim`` has the definition, ``ops.ref_fim_tokens``): the emit launch renders its ids into a scratch area at
the end of the step's window and writes no labels, and ``token_fim`` -- one more launch on the prep stream -- writes
the batch's ``input_ids`` and ``labels``. A segment's key is the plan's ``seg_src``, the corpus element of its first
token, and the epoch's key follows from ``seed`` and the epoch: the rearrangement does not depend on the world size,
the rank, ``shuffle_rows``, the batch a row lands in or where the tokens lie. With a ``mix``, two copies of a
document in one epoch get the same cuts where their pieces start at the same token. Without ``fim`` the launches,
buffers and bytes are unchanged.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _native
from .corpus_replica import ResidentCorpusLoader
from .exceptions import DDLError
from .models.tokens import SharedTokenSource
from .ops.kernels import (_align16, _stream_seg_keys, check_ignore_index, launch_mix_order, launch_stream_plan,
                          launch_stream_plan_rows, ref_fim_tokens, ref_mix_order, ref_stream_tokens, row_selector,
                          stream_max_segments, token_stream_bytes)
from .permutation import FeistelPermutation, row_seed_for
from .resident import STATE_VERSION, PrefetchedIndexedLoader
from .token_fim import TokenFIM
from .token_mix import TokenMix
from .types import DDLEnv
from .utils import streams


class _RowOrder:
    """What ``PrefetchedIndexedLoader`` asks of an order, over the rows of the stream."""

    def __init__(self, rows_per_epoch: int, global_batch: int, seed: int, shuffle: bool):
        self.n_samples, self.global_batch, self.seed, self.shuffle = rows_per_epoch, global_batch, seed, shuffle
        self.batches_per_epoch = rows_per_epoch // global_batch


class TokenStreamLoader(ResidentCorpusLoader, PrefetchedIndexedLoader):
    """What the loaders of the stream format share: the epoch's order, tables and selectors, the step, the
    ``kind="token_stream"`` checkpoint. A loader says where the device reads the corpus and its offsets
    (``_corpus_ptr``, ``_offsets_dev``), which launch path renders a step (``_launch_plan`` / ``_launch_plan_rows``
    with ``_launch_kw``) and how large a step's window between the launches is (``_window_bytes``)."""

    _launch_plan = staticmethod(launch_stream_plan)
    _launch_plan_rows = staticmethod(launch_stream_plan_rows)
    _corpus_ptr = 0        # the address the device reads the corpus's tokens at
    _offsets_dev = None    # the corpus offsets in HBM

    def _launch_kw(self) -> dict:
        return {}

    def _window_bytes(self) -> int:
        return self._plan_bytes + self._fim_bytes

    def _init_stream(self, source: SharedTokenSource, global_batch: int, seq_len: int, env: DDLEnv | None, *,
                     seed: int, shuffle: bool, pad_id: int, depth: int, device, n_epochs: int | None,
                     resume_state: dict | None, handoff: str, max_segments: int | None, labels: bool,
                     ignore_index: int, shuffle_rows: bool, mix: TokenMix | None,
                     fim: TokenFIM | None = None) -> None:
        """The arguments checked, the epoch's sizes, the cursor and the prep stream: everything in front of the
        corpus itself."""
        if handoff not in ("device", "host"):
            raise ValueError("handoff must be 'device' or 'host'")
        self.labels, self.ignore_index = bool(labels), check_ignore_index(labels, ignore_index)
        self.handoff = handoff
        self.env = env or DDLEnv()
        self.W, self.rank = self.env.world_size, self.env.rank
        self.source, self.seq_len, self.pad_id = source, int(seq_len), int(pad_id)
        self.GB = int(global_batch)
        if self.seq_len <= 0 or self.GB <= 0:
            raise ValueError("seq_len and global_batch must be positive")
        if self.GB % self.W:
            raise ValueError(f"global batch {self.GB} not divisible by world size {self.W}")
        self.LB = self.GB // self.W
        if self.LB * self.seq_len > 0x7FFFFFFF:
            raise ValueError(f"{self.LB} rows of {self.seq_len} tokens overflow int32 cu_seqlens")
        self._toks = source.tokens.tensor().view(-1)  # keeps the mappings alive
        self._offs_t = source.offsets.tensor().view(-1)
        offs = self._offs_t.numpy()
        lens = np.maximum(np.diff(offs), 0)
        self.n_documents, self.total_tokens = int(source.n), int(lens.sum())
        if fim is not None and not isinstance(fim, TokenFIM):
            raise TypeError("fim must be a TokenFIM")
        self.fim = fim
        # the ids the emit launch renders for token_fim to rearrange: a scratch area at the end of a step's window
        self._fim_bytes = _align16(4 * self.LB * self.seq_len) if fim is not None else 0
        self.mix = mix
        if mix is not None:
            if not isinstance(mix, TokenMix):
                raise TypeError("mix must be a TokenMix")
            if mix.n_documents != self.n_documents:
                raise ValueError(f"the mix covers {mix.n_documents} documents, the corpus has {self.n_documents}")
            self.total_tokens = mix.epoch_tokens(lens, int(seed), bool(shuffle))
            lens = np.repeat(lens, mix.document_copies())
        self.n_order = mix.n_order if mix is not None else self.n_documents
        if self.total_tokens < self.GB * self.seq_len:
            raise ValueError(f"an epoch holds {self.total_tokens} tokens, fewer than one global batch of "
                             f"{self.GB} x {self.seq_len}")
        self.order = _RowOrder(self.total_tokens // self.seq_len, self.GB, int(seed), bool(shuffle))
        self.shuffle_rows = bool(shuffle_rows)
        self.row_seed = row_seed_for(seed)
        self.max_segments = (stream_max_segments(lens, self.LB, self.seq_len, self.shuffle_rows)
                             if max_segments is None else int(max_segments))
        if self.max_segments < 1:
            raise ValueError("max_segments must be >= 1")
        self._max_seqlen = min(self.seq_len, int(source.max_len))
        self.out_dtype = torch.int32
        self.device = self._resolve_device(self.env, device)
        self._init_cursor(seed, depth, n_epochs, resume_state)
        self.nbytes = int(offs[-1]) * source.token_bytes if source.n else 0
        self.n_elems = self.nbytes // source.token_bytes
        self.prep_stream = streams.batch_stream(self.device) if self.device.type == "cuda" else None
        self.tables_built = self.orders_built = 0
        self._epoch_evs: list = []
        self._windows: list = []

    def _table_bytes(self) -> int:
        """Bytes of the two epoch tables, the scan's scratch and (a mix) the two orders."""
        n = self.n_order
        scratch = _native.hip().token_stream_table_scratch(n)
        return 8 * (2 * (n + 1) + scratch + (2 * n if self.mix is not None else 0))

    def _init_tables(self) -> None:
        """The two tables, the orders of a mix and the ring of windows, on the prep stream."""
        n, mix = self.n_order, self.mix
        scratch = _native.hip().token_stream_table_scratch(n)
        with streams.on_stream(self.prep_stream):
            # two tables: prefetch crosses the epoch boundary (epoch e lives in slot e % 2)
            self._tables = [torch.empty(n + 1, dtype=torch.int64, device=self.device) for _ in range(2)]
            self._scratch = torch.empty(scratch, dtype=torch.int64, device=self.device)
            self._table_epoch = [None, None]
            if mix is not None:  # the epochs' document orders, slot for slot with the tables
                self._orders = [torch.empty(n, dtype=torch.int64, device=self.device) for _ in range(2)]
                self._order_sel = [row_selector(o) for o in self._orders]
                self._mix_args = mix.device_args(self.seed, self.order.shuffle)
            self._plan_bytes, self._batch_bytes = token_stream_bytes(self.LB, self.seq_len, self.max_segments,
                                                                     labels=self.labels,
                                                                     shuffled_rows=self.shuffle_rows)
            self._windows = [torch.empty(self._window_bytes(), dtype=torch.uint8, device=self.device)
                             for _ in range(self.depth + 1)]

    # ---------------------------------------------------------------- order
    def _perm(self, epoch: int) -> FeistelPermutation | None:
        return FeistelPermutation(self.n_documents, self.seed, epoch) if self.order.shuffle else None

    def _mix_perm(self, epoch: int) -> FeistelPermutation | None:
        return FeistelPermutation(self.n_order, self.seed, epoch) if self.order.shuffle else None

    def _row_perm(self, epoch: int) -> FeistelPermutation | None:
        return FeistelPermutation(self.order.n_samples, self.row_seed, epoch) if self.shuffle_rows else None

    def _order(self, epoch: int) -> np.ndarray | None:
        """The CPU twin's document order of a mix (None without one: ``_perm`` is the order)."""
        if self.mix is None:
            return None
        return ref_mix_order(self.mix, seed=self.seed, epoch=epoch, shuffle=self.order.shuffle)

    def _doc_selector(self, epoch: int) -> dict:
        """The ``RowIndex`` of the epoch's documents: its permutation, or the slot's order buffer of a mix."""
        return self._selector(epoch) if self.mix is None else self._order_sel[epoch % 2]

    def _table(self, epoch: int, sel: dict) -> torch.Tensor:
        """Epoch ``epoch``'s table (behind its order, with a mix), built on the prep stream the first time a step
        of the epoch is assembled. The slot's earlier epoch is two behind: every step that reads it was enqueued
        before."""
        k = epoch % 2
        if self._table_epoch[k] != epoch:
            timed = self.profile_every > 0
            if timed:  # the epoch's launches between two timing events (``timing``)
                evs = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                evs[0].record(self.prep_stream)
            if self.mix is not None:
                launch_mix_order(_native.hip(), self._orders[k].data_ptr(), self._mix_args,
                                 n_corpus=self.n_documents, n=self.n_order, perm=self._mix_perm(epoch),
                                 stream=self.prep_stream.cuda_stream)
                self.orders_built += 1
            _native.hip().token_stream_table(
                corpus_offsets=self._offsets_dev.data_ptr(), n_corpus=self.n_documents, n=self.n_order,
                table=self._tables[k].data_ptr(), tile_sums=self._scratch.data_ptr(),
                stream=self.prep_stream.cuda_stream, **sel)
            if timed:
                evs[1].record(self.prep_stream)
                self._epoch_evs.append(evs)
            self._table_epoch[k] = epoch
            self.tables_built += 1
        return self._tables[k]

    def _step(self, t: int):
        e, g = divmod(t, self.order.batches_per_epoch)
        row_base = g * self.GB + self.rank * self.LB
        st = self.prep_stream
        if st is None:  # the CPU twin: the definition itself
            r = ref_stream_tokens(self._toks, self._offs_t, perm=self._perm(e) if self.mix is None else None,
                                  row_base=row_base, rows=self.LB, seq_len=self.seq_len, pad_id=self.pad_id,
                                  max_segs=self.max_segments, labels=self.labels and self.fim is None,
                                  ignore_index=self.ignore_index, row_perm=self._row_perm(e), order=self._order(e))
            if self.fim is not None:
                keys = _stream_seg_keys(self._offs_t, r, perm=self._perm(e) if self.mix is None else None,
                                           order=self._order(e), row_base=row_base, seq_len=self.seq_len,
                                           row_perm=self._row_perm(e))
                r = ref_fim_tokens(r, self.fim, seg_keys=keys, seed=self.seed, epoch=e, labels=self.labels,
                                   ignore_index=self.ignore_index)
            ev = None
        else:
            sel = self._doc_selector(e)
            table = self._table(e, sel)

            def issue(win, whole):
                common = dict(
                    corpus_ptr=self._corpus_ptr, corpus_elems=self.n_elems,
                    tok16=self.source.token_bytes == 2, corpus_offsets_ptr=self._offsets_dev.data_ptr(),
                    n_corpus=self.n_documents, n=self.n_order, table_ptr=table.data_ptr(), selector=sel,
                    rows=self.LB, seq_len=self.seq_len, pad_id=self.pad_id, max_segs=self.max_segments,
                    stream=st.cuda_stream, labels=self.labels, ignore_index=self.ignore_index, **self._launch_kw())
                if self.fim is not None:
                    common["fim"] = {"scratch_ptr": win.data_ptr() + self._window_bytes() - self._fim_bytes,
                                     "args": self.fim.device_args(self.seed, e)}
                if self.shuffle_rows:
                    return self._launch_plan_rows(
                        win.data_ptr(), whole, stream_rows=self.order.n_samples,
                        row_selector=dict(self._selector(e, self._row_perm), base=row_base), **common)
                return self._launch_plan(win.data_ptr(), whole, row_base=row_base, **common)

            r, ev = self._launch(t, self._batch_bytes, issue)
        counts = r.pop("counts")
        r["max_seqlen"] = self._max_seqlen  # a static upper bound (varlen attention accepts one)
        r["n_tokens"], r["n_rows"], r["n_seg"] = counts[2], counts[0], counts[1]
        return r, ev

    # ----------------------------------------------------------- checkpoint
    def state_dict(self) -> dict:
        return {
            "version": STATE_VERSION,
            "kind": "token_stream",
            "seed": self.seed,
            "order_seed": self.seed,
            "epoch": self.epoch,
            "global_batch_cursor": self.cursor + (1 if self._pending else 0),
            "batches_per_epoch": self.order.batches_per_epoch,
            "global_batch": self.GB,
            "seq_len": self.seq_len,
            "n_documents": self.n_documents,
            "total_tokens": self.total_tokens,
            "shuffle": self.order.shuffle,
            "shuffle_rows": self.shuffle_rows,
            "row_seed": self.row_seed,
            "world_size": self.W,
            "mix": None if self.mix is None else self.mix.state(),
            "n_order": self.n_order,
            "fim": None if self.fim is None else self.fim.state(),
        }

    def _apply_state(self, sd: dict) -> None:
        if sd.get("kind") != "token_stream" or sd.get("version") != STATE_VERSION:
            raise ValueError(f"not a token stream loader state (kind={sd.get('kind')!r}): rows of the token stream "
                             "and batches of sequences do not share a cursor")
        mix_state = None if self.mix is None else self.mix.state()
        if sd.get("mix") != mix_state:  # a state without the key: no mix; before total_tokens, which a mix changes
            raise ValueError(f"checkpoint mix={sd.get('mix')} does not match {mix_state}")
        fim_state = None if self.fim is None else self.fim.state()
        if sd.get("fim") != fim_state:  # a state without the key: no FIM
            raise ValueError(f"checkpoint fim={sd.get('fim')} does not match {fim_state}")
        for key, mine in (("global_batch", self.GB), ("seq_len", self.seq_len), ("n_documents", self.n_documents),
                          ("total_tokens", self.total_tokens), ("order_seed", self.seed),
                          ("shuffle", self.order.shuffle), ("n_order", self.n_order)):
            if sd.get(key) is not None and sd[key] != mine:
                raise ValueError(f"checkpoint {key}={sd[key]} does not match {mine}")
        if bool(sd.get("shuffle_rows", False)) != self.shuffle_rows:  # a state without the key: contiguous rows
            raise ValueError(f"checkpoint shuffle_rows={bool(sd.get('shuffle_rows', False))} does not match "
                             f"{self.shuffle_rows}")
        if self.shuffle_rows and sd.get("row_seed") != self.row_seed:
            raise ValueError(f"checkpoint row_seed={sd.get('row_seed')} does not match {self.row_seed}")
        self.epoch, self.cursor = int(sd["epoch"]), int(sd["global_batch_cursor"])
        if self.cursor >= self.order.batches_per_epoch:
            self.epoch, self.cursor = self.epoch + 1, 0

    # ---------------------------------------------------------------- misc
    def timing(self) -> dict:
        """``ResidentCorpusLoader.timing`` and ``epoch_prep_us``: the mean device time of an epoch's own launches
        (``token_mix_order`` with a mix, and the table scan) over the epochs begun while ``profile_every`` > 0."""
        out = super().timing()
        evs = self._epoch_evs
        out["epoch_prep_us"], out["epoch_prep_samples"] = None, len(evs)
        if evs:
            self.prep_stream.synchronize()
            out["epoch_prep_us"] = 1e3 * sum(a.elapsed_time(b) for a, b in evs) / len(evs)
        return out

    def _close_stream(self) -> None:
        """Drain the prep stream and drop the queue, the windows, the tables and the orders."""
        if getattr(self, "prep_stream", None) is not None:
            self.prep_stream.synchronize()
        if hasattr(self, "_queue"):
            self._queue.clear()
        self._kernel_evs = []
        self._windows = []
        self._tables = self._scratch = self._orders = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


class ResidentTokenStreamLoader(TokenStreamLoader):
    def __init__(self, source: SharedTokenSource, global_batch: int, seq_len: int = 4096, env: DDLEnv | None = None,
                 *, seed: int = 0, shuffle: bool = True, pad_id: int = 0, depth: int = 2,
                 device: str | torch.device | None = None, n_epochs: int | None = None,
                 resume_state: dict | None = None, handoff: str = "device", hbm_fraction: float = 0.8,
                 chunk_bytes: int = 256 << 20, max_segments: int | None = None, labels: bool = False,
                 ignore_index: int = -100, shuffle_rows: bool = False, mix: TokenMix | None = None,
                 fim: TokenFIM | None = None):
        """``global_batch`` counts rows. ``max_segments``: the capacity of a batch's ``cu_seqlens`` (default
        ``ops.stream_max_segments``, which no window of any order exceeds; a smaller one that a batch overflows
        gives that batch as padding with ``n_rows`` = -1). ``shuffle_rows``: the rows of an epoch in the order of
        a second permutation (see the module's text); ``shuffle=False`` with it gives shuffled rows of the
        unshuffled stream. ``mix``: a ``TokenMix`` over all the corpus's documents (``mix.bounds[-1] ==
        n_documents``): the epoch's documents are its weighted order. The extra documents of a fractional repeat
        are the same in every epoch, so ``total_tokens`` -- the tokens of one epoch, computed here once -- and
        with it the rows and batches per epoch and the checkpoint cursor are constants; the default
        ``max_segments`` is ``ops.stream_max_segments`` over the lengths with every document counted
        ``mix.max_copies`` times, a multiset that holds every epoch's documents. ``fim``: a ``TokenFIM``, the
        fill-in-the-middle rearrangement of a share of every batch's segments (the module's text)."""
        self._init_stream(source, global_batch, seq_len, env, seed=seed, shuffle=shuffle, pad_id=pad_id, depth=depth,
                          device=device, n_epochs=n_epochs, resume_state=resume_state, handoff=handoff,
                          max_segments=max_segments, labels=labels, ignore_index=ignore_index,
                          shuffle_rows=shuffle_rows, mix=mix, fim=fim)
        if not self._attach_replica(hbm_fraction, chunk_bytes):
            return
        try:
            table_bytes = self._table_bytes()
            free, _ = torch.cuda.mem_get_info(self.device)
            if table_bytes > float(hbm_fraction) * free:
                raise DDLError(f"the two epoch tables{' and orders' if mix is not None else ''} ({table_bytes} bytes) "
                               f"exceed hbm_fraction={hbm_fraction} of the free HBM ({free} bytes free)")
            self._offsets_dev = self._replica.offsets(self._offs_t, self.prep_stream)
            self._corpus_ptr = self._replica.hbm.data_ptr()
            self._init_tables()
        except Exception:
            self.close()
            raise

    def stats(self) -> dict:
        return {"batches": self.batches, "source_bytes": self.nbytes, "load_s": self.load_s,
                "load_gbps": self.nbytes / self.load_s / 1e9 if self.load_s > 0 else 0.0, "handoff": self.handoff,
                "host_waits": self.host_waits, "replica_shared": self.replica_shared, "format": "stream",
                "rows_per_epoch": self.order.n_samples, "max_segments": self.max_segments,
                "tables_built": self.tables_built, "shuffle_rows": self.shuffle_rows,
                "mix_parts": self.mix.parts if self.mix is not None else 0, "mix_documents": self.n_order,
                "orders_built": self.orders_built, "fim": self.fim is not None}

    def close(self) -> None:
        self._close_stream()
        self._release_replica()
