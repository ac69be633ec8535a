#!/usr/bin/env python3
"""Packed (or padded) token batches for LLM training, seq_len 4096 (BASELINE config 4).

    python examples/tokens_packed.py [--mode pad]
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 examples/tokens_packed.py

A tokenised corpus (flat int32 tokens + int64 sequence offsets) sits in node-shared
memory (``SharedTokenSource``; ``.create(name, tokens, offsets)`` for your own data).
Producers gather each step's sequences in the world-size-invariant global order
and ship them RAGGED, so only real tokens cross PCIe. The consumer expands a
batch on the GPU with the pad/pack kernel:

* ``pack``: sequences packed into rows of ``seq_len`` by first-fit decreasing
  (``pack_order="ffd"``, ~93% dense measured; long ones split).
  Returns ``input_ids``, ``attention_mask``, ``position_ids`` (restarting per
  sequence), ``segment_ids``, int32 ``cu_seqlens`` over ``input_ids[attention_mask.bool()]`` and
  ``max_seqlen`` (the varlen-attention inputs; one entry per segment).
* ``pad``: one sequence per row, padded with ``pad_id``.

``batches_per_window=k`` ships k consecutive global batches per producer window
(one producer round, one H2D copy and one stager hand-off per k batches).

``--zero-copy`` needs no producers: ``ZeroCopyTokenLoader`` registers the corpus once and a gfx950 kernel
gathers each batch's ragged sequences straight out of it over PCIe (no host copy; every token is read from
DRAM once). Same batches, same checkpoint.

``--resident`` needs no producers and no link either: ``ResidentTokenLoader`` copies the corpus into HBM once (it
must fit: 2-4 bytes per token) and one gfx950 kernel packs every batch straight out of it. Same batches, same
checkpoint. ``DDL_DEVICE=cpu`` runs it (and ``--zero-copy``) with the host twin.

``--resident --device-plan`` also builds each batch's order and pack plan on the GPU (``plan="device"``): the host
only issues launches. Packing is in-order, shapes are static (fixed rows, ``cu_seqlens`` of fixed capacity) and
``n_tokens`` / ``n_rows`` / ``n_seg`` are 0-d device tensors; ``max_seqlen`` is an upper bound. ``--ffd`` adds the
first-fit-decreasing order to that mode (``pack_order="ffd_device"``: one more kernel, the batches of the host FFD
plan, at most 4096 sequences per rank and step).

``--resident --stream`` delivers the GPT pre-training format instead (``ResidentTokenStreamLoader``): the epoch's
shuffled documents concatenated and cut every ``seq_len`` tokens, so ``--global-batch`` counts ROWS, every row is
full (100% dense, static shapes) and a segment is a run of one document inside one row. The stream's table and
each batch's plan are built on the GPU; the checkpoint is ``kind="token_stream"``. ``--shuffle-rows`` adds the
sample shuffle of that format (Megatron's ``shuffle_idx``): a step's rows are drawn from all over the epoch's
stream by a second permutation, so the pieces of a long document no longer sit in neighbouring rows of one step.
``--mix 2,1,0.5`` weights parts of the corpus (``ddl_amd.TokenMix``): the documents are cut into as many equal
parts as there are numbers, and a document of part ``p`` appears ``repeat[p]`` times per epoch (a fraction: that
share of the part's documents once more, the same ones every epoch).
``--fim 0.5`` rearranges that share of the segments for fill-in-the-middle training (``ddl_amd.TokenFIM``, by a
kernel behind the emit launch): ``<PRE> prefix <SUF> suffix <MID> middle`` or its SPM form, with the three sentinel
ids just past the vocabulary; labels follow the rearranged ids.

``--zero-copy --stream`` delivers the same format from a corpus that stays in host memory
(``ZeroCopyTokenStreamLoader``): only the offsets are uploaded, each batch's pieces are read over PCIe by
``gather_stream_pieces`` and the batches, ``--shuffle-rows``, ``--mix``, ``--labels`` and the checkpoint are those of
``--resident --stream``.

``--labels`` (with ``--resident`` or ``--zero-copy``) asks the loader for the next-token targets as well
(``labels=True``: int64 ``labels``, ``-100`` where a position has no target -- the end of a row or of a segment,
padding) and trains a toy embedding + linear model on every batch with ``cross_entropy(ignore_index=-100)``.

``state_dict()`` is the indexed-kind cursor (seed, epoch, global batch), so a
job can resume at another world size.
"""

import argparse
import os

import torch

import ddl_amd
from ddl_amd.models.tokens import SharedTokenSource, TokenBatchProducer


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="pack", choices=["pack", "pad"])
    ap.add_argument("--n-seqs", type=int, default=1024)
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--global-batch", type=int, default=32, help="sequences per global step")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batches-per-window", type=int, default=4)
    ap.add_argument("--zero-copy", action="store_true",
                    help="no producers: the GPU gathers the batches out of the registered corpus")
    ap.add_argument("--resident", action="store_true",
                    help="no producers, no PCIe per step: the corpus lives in HBM and one kernel packs the batches")
    ap.add_argument("--device-plan", action="store_true",
                    help="with --resident: the batch's order and pack plan are built on the GPU too (in-order "
                         "packing, static shapes, counts as device scalars)")
    ap.add_argument("--ffd", action="store_true",
                    help="with --resident --device-plan --mode pack: first-fit-decreasing rows, ordered by a kernel "
                         "(pack_order='ffd_device')")
    ap.add_argument("--stream", action="store_true",
                    help="with --resident or --zero-copy: full rows cut from the concatenated shuffled documents "
                         "(--global-batch counts rows)")
    ap.add_argument("--shuffle-rows", action="store_true",
                    help="with --stream: the epoch's rows in a shuffled order (shuffle_rows=True)")
    ap.add_argument("--mix", default=None, metavar="R0,R1,...",
                    help="with --stream: repeats of equal parts of the corpus, e.g. 2,1,0.5 (TokenMix)")
    ap.add_argument("--fim", type=float, default=None, metavar="RATE",
                    help="with --stream: the share of segments rearranged for fill-in-the-middle (TokenFIM)")
    ap.add_argument("--labels", action="store_true",
                    help="with --resident or --zero-copy: the loader also delivers next-token labels, and every "
                         "batch runs a tiny embedding -> linear -> cross_entropy step on them")
    ap.add_argument("--vocab", type=int, default=None,
                    help="vocabulary of the synthetic corpus (default 50257; 512 with --labels, whose toy model "
                         "holds [positions, vocab] logits)")
    a = ap.parse_args()
    if a.zero_copy and a.resident:
        ap.error("--zero-copy and --resident are two loaders: pick one")
    if a.device_plan and not a.resident:
        ap.error("--device-plan is a mode of --resident")
    if a.ffd and (not a.device_plan or a.mode != "pack"):
        ap.error("--ffd is an option of --resident --device-plan --mode pack")
    if a.stream and (not (a.resident or a.zero_copy) or a.device_plan or a.mode != "pack"):
        ap.error("--stream is a format of --resident and --zero-copy (packed rows by construction; it has no "
                 "--device-plan mode)")
    if a.shuffle_rows and not a.stream:
        ap.error("--shuffle-rows is an option of --stream")
    if a.mix and not a.stream:
        ap.error("--mix is an option of --stream")
    if a.fim is not None and not a.stream:
        ap.error("--fim is an option of --stream")
    if a.labels and not (a.zero_copy or a.resident):
        ap.error("--labels needs --resident or --zero-copy (the producer path does not deliver labels)")
    vocab = a.vocab or (512 if a.labels else 50257)
    lab_kw = dict(labels=True, ignore_index=-100) if a.labels else {}

    name = f"ddl_amd_example_tok_{os.environ.get('MASTER_PORT', os.getpid())}"
    creator = int(os.environ.get("LOCAL_RANK", "0")) == 0
    src = SharedTokenSource.synthetic(name, a.n_seqs, 64, a.seq_len, vocab=vocab, seed=0) if creator else None
    try:
        with ddl_amd.start(n_producers=0 if (a.zero_copy or a.resident) else 2) as (env, conn):
            if env.world_size > 1:
                torch.distributed.barrier(group=env.control_group)
            if src is None:  # other local ranks attach to the creator's segments
                from ddl_amd.models import SharedArraySource

                offs = SharedArraySource(name + "_off", a.n_seqs + 1, (1,), "int64")
                n_tok = int(offs.tensor()[-1])
                src = SharedTokenSource(SharedArraySource(name + "_tok", n_tok, (1,), "int32"), offs, a.seq_len)
            pack_order = "ffd" if a.mode == "pack" else "in_order"
            if a.stream:
                mix = None
                if a.mix:  # equal parts of the corpus, by document index
                    repeat = [float(r) for r in a.mix.split(",")]
                    bounds = [round(p * a.n_seqs / len(repeat)) for p in range(len(repeat) + 1)]
                    mix = ddl_amd.TokenMix(bounds, repeat)
                fim = None
                if a.fim is not None:  # the sentinels just past the vocabulary
                    fim = ddl_amd.TokenFIM(a.fim, prefix_id=vocab, middle_id=vocab + 1, suffix_id=vocab + 2)
                stream_cls = ddl_amd.ResidentTokenStreamLoader if a.resident else ddl_amd.ZeroCopyTokenStreamLoader
                dl = stream_cls(src, a.global_batch, a.seq_len, env, n_epochs=a.epochs, shuffle_rows=a.shuffle_rows,
                                mix=mix, fim=fim, **lab_kw)
                if mix is not None and env.rank == 0:
                    print(f"mix: {mix.parts} parts x {list(mix.repeat)} -> {mix.n_order} documents and "
                          f"{dl.total_tokens} tokens per epoch (the corpus: {a.n_seqs} documents)", flush=True)
            elif a.resident and a.device_plan:  # in-order, or first-fit-decreasing built by a kernel
                dl = ddl_amd.ResidentTokenLoader(src, a.global_batch, a.seq_len, a.mode, env, n_epochs=a.epochs,
                                                 plan="device", pack_order="ffd_device" if a.ffd else "in_order",
                                                 **lab_kw)
            elif a.resident:
                dl = ddl_amd.ResidentTokenLoader(src, a.global_batch, a.seq_len, a.mode, env, pack_order=pack_order,
                                                 n_epochs=a.epochs, **lab_kw)
            elif a.zero_copy:
                dl = ddl_amd.ZeroCopyTokenLoader(src, a.global_batch, a.seq_len, a.mode, env, pack_order=pack_order,
                                                 n_epochs=a.epochs, **lab_kw)
            else:
                producer = TokenBatchProducer(src, a.global_batch, a.seq_len, a.mode, pack_order=pack_order,
                                              batches_per_window=a.batches_per_window)
                dl = ddl_amd.DistributedDataLoader(producer, a.global_batch // env.world_size, conn, a.epochs,
                                                   env=env, order=ddl_amd.OrderSpec(mode="indexed"),
                                                   output=ddl_amd.OutputSpec(collate="tokens"), auto_mark=True)
            if a.labels:  # a toy causal-LM step: the loader's labels are what cross_entropy takes, as they come
                torch.manual_seed(0)
                n_ids = vocab + (3 if a.fim is not None else 0)  # the FIM sentinels are ids of their own
                model = torch.nn.Sequential(torch.nn.Embedding(n_ids, 32), torch.nn.Linear(32, n_ids)).to(dl.device)
                opt = torch.optim.SGD(model.parameters(), lr=0.1)
            for epoch in range(a.epochs):
                real = rows = 0
                for step, b in enumerate(dl):
                    if a.fim is not None and epoch == 0 and step == 0 and env.rank == 0:
                        first = (b["position_ids"] == 0) & (b["attention_mask"] != 0)  # every segment's first token
                        moved = int((b["input_ids"][first] == vocab).sum())
                        print(f"fim: {moved} of {int(first.sum())} segments rearranged in the first batch "
                              f"({100.0 * moved / max(int(first.sum()), 1):.1f}%, rate {a.fim})", flush=True)
                    real += int(b["attention_mask"].sum())
                    rows += int(b.get("n_rows", b["input_ids"].shape[0]))  # fixed rows: the packed ones
                    if a.labels:
                        logits = model(b["input_ids"])
                        loss = torch.nn.functional.cross_entropy(logits.view(-1, n_ids), b["labels"].view(-1),
                                                                 ignore_index=-100)
                        opt.zero_grad(set_to_none=True)
                        loss.backward()
                        opt.step()
                if a.labels and env.rank == 0:
                    print(f"epoch {epoch}: loss {loss.item():.4f} over "
                          f"{int((b['labels'] != -100).sum())} targets of the last batch", flush=True)
                if env.rank == 0:
                    # cu_seqlens has one entry per SEGMENT: over-long sequences are split into seq_len chunks
                    # and empty sequences have none, so this is not the sequence count
                    n_seg = int(b["n_seg"]) if "n_seg" in b else b["cu_seqlens"].numel() - 1 if a.mode == "pack" else 0
                    extra = (f", {n_seg} segments (max {b['max_seqlen']} tokens) in the last batch"
                             if a.mode == "pack" else "")
                    print(f"epoch {epoch}: {rows} rows x {a.seq_len} on rank 0, {real} real tokens "
                          f"({100.0 * real / max(rows * a.seq_len, 1):.1f}% dense){extra}; keys {sorted(b)}",
                          flush=True)
            if a.resident and env.rank == 0:
                st = dl.stats()
                where = f"in HBM, loaded in {st['load_s']:.3f} s" if st["load_s"] else "read in place (CPU twin)"
                print(f"resident corpus: {st['source_bytes']} bytes {where}, hand-off {st['handoff']}", flush=True)
            if a.zero_copy or a.resident:
                dl.close()
    finally:
        if src is not None:
            src.close()


if __name__ == "__main__":
    main()
