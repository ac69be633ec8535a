#!/usr/bin/env python3
"""BASELINE config 4: token sequences, seq_len=4096, ragged H2D + on-device pad/pack collate.

Synthetic corpus (random token ids, lengths uniform in [min_len, 4096]) in node
shm; producers gather sequences in the world-size-invariant global order into
pinned windows (ragged: only real tokens cross PCIe); the consumer expands
them with the gfx950 pad_pack_tokens kernel. Reports tokens/s fed to the GPU
(real tokens, padding excluded) and batches/s. torchrun-compatible.
"""

import argparse
import json
import os
import sys
import time

import numpy as np


def _fim_report(a, stream_loader, fim, dev):
    """``--fim``: the stream loader without and with FIM in turns (fresh loaders, this rank's batches: real tokens per
    second of wall time behind a device synchronise, and the mean device time of a step's launches), and the
    ``token_fim`` kernel alone between device events on one rendered batch, next to a device copy of as many bytes as
    the kernel reads and writes (4 B ids, 4 B segment ids and 8 B position ids read, 4 B ids and, with labels, 8 B
    written per position)."""
    import torch

    from ddl_amd import _native
    from ddl_amd.ops.kernels import launch_fim

    runs = []
    for turn in range(4):
        dl = stream_loader(fim if turn % 2 else None)

        def gen():
            while True:
                yield from dl

        it = gen()
        for _ in range(a.warmup):
            next(it)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        real = torch.zeros((), dtype=torch.int64, device=dev)
        for _ in range(a.steps):
            real.add_(next(it)["n_tokens"])
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        timing = dl.timing()
        runs.append({"fim": bool(turn % 2), "tokens_per_s": round(int(real) / dt, 1),
                     "ms_per_step": round(1e3 * dt / a.steps, 4),
                     "kernel_us": None if timing["kernel_us"] is None else round(timing["kernel_us"], 1),
                     "kernel_samples": timing["kernel_samples"]})
        if turn == 3:  # the kernel alone, on the last delivered batch of the FIM loader's plain twin
            dl.close()
            dl = stream_loader(None)
            b = next(iter(dl))
            R, S = b["input_ids"].shape
            keys = torch.arange(b["cu_seqlens"].numel() - 1, dtype=torch.int64, device=dev) * 977
            out = torch.empty((R, S), dtype=torch.int32, device=dev)
            lab = torch.empty((R, S), dtype=torch.int64, device=dev) if a.labels else None
            moved = R * S * (4 + 4 + b["position_ids"].element_size() + 4 + (8 if a.labels else 0))
            src_buf = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst_buf = torch.empty_like(src_buf)
            stream = torch.cuda.current_stream(dev).cuda_stream
            h = _native.hip()

            def fim_launch():
                launch_fim(h, ids_ptr=b["input_ids"].data_ptr(), seg=b["segment_ids"], pos=b["position_ids"],
                           cu_ptr=b["cu_seqlens"].data_ptr(), cap=keys.numel(), seg_keys_ptr=keys.data_ptr(),
                           counts_ptr=0, out_ptr=out.data_ptr(), labels_ptr=lab.data_ptr() if a.labels else 0,
                           ignore_index=-100, rows=R, seq_len=S, fim_args=fim.device_args(0, 0), stream=stream)

            def timed(fn, n=200):
                for _ in range(20):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
                torch.cuda.synchronize(dev)
                return 1e3 * e0.elapsed_time(e1) / n

            torch.cuda.synchronize(dev)
            k_us = [timed(fim_launch), timed(lambda: dst_buf.copy_(src_buf)), timed(fim_launch),
                    timed(lambda: dst_buf.copy_(src_buf))]
            kernel = {"rows": R, "seq_len": S, "labels": bool(a.labels), "bytes_moved": moved,
                      "token_fim_us": [round(k_us[0], 2), round(k_us[2], 2)],
                      "copy_same_bytes_us": [round(k_us[1], 2), round(k_us[3], 2)],
                      "token_fim_tbps": round(moved / min(k_us[0], k_us[2]) / 1e6, 3),
                      "copy_tbps": round(moved / min(k_us[1], k_us[3]) / 1e6, 3)}
        dl.close()
    return {"rate": a.fim, "runs": runs, "kernel": kernel}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64, help="sequences per rank per step")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--min-len", type=int, default=256)
    ap.add_argument("--n-seqs", type=int, default=8192)
    ap.add_argument("--producers", type=int, default=6)
    ap.add_argument("--slots", type=int, default=2, help="windows per producer (a producer fills one while the "
                                                          "previous is in flight)")
    ap.add_argument("--batches-per-window", type=int, default=8,
                    help="global batches per producer window (per-window costs amortised over k batches)")
    ap.add_argument("--host-threads", type=int, default=4, help="gather threads per producer")
    ap.add_argument("--token-rows", default="exact", choices=["exact", "fixed"],
                    help="pack mode: exact packed rows per batch, or the window layout's fixed max rows (padding)")
    ap.add_argument("--dispatch", default="auto", choices=["auto", "inline", "lookahead", "window", "python"])
    ap.add_argument("--mode", default="pack", choices=["pad", "pack"])
    ap.add_argument("--max-rows", type=int, default=None,
                    help="--path resident --plan device --mode pack: the static row count of every batch "
                         "(default: the worst case)")
    ap.add_argument("--pack-order", default="ffd", choices=["in_order", "ffd", "ffd_device"],
                    help="pack mode: first-fit-decreasing rows (measured 93%% dense) or in-order (~75%%)")
    ap.add_argument("--idle-steps", type=int, default=200,
                    help="phase 2: steps of a fixed-cost token train step, for GPU idle %% (0 disables)")
    ap.add_argument("--model-dim", type=int, default=256)
    ap.add_argument("--model-depth", type=int, default=2)
    ap.add_argument("--token-dtype", default="auto", choices=["auto", "int32", "uint16"],
                    help="token ids in the corpus and on the wire: auto = uint16 when every id is < 65536 (the "
                         "synthetic GPT-2-sized vocabulary is), else int32; uint16 ships 2 B per token over PCIe "
                         "and the pack kernel widens it to int32 input_ids (archive/profiles/r3_tok16)")
    ap.add_argument("--path", default="producers", choices=["producers", "zerocopy", "resident"],
                    help="producers: host producers gather into pinned windows (TokenBatchProducer); zerocopy: the "
                         "ragged gather kernel reads the registered corpus over PCIe (ZeroCopyTokenLoader); resident: "
                         "the corpus is copied into HBM once and one kernel packs every batch out of it "
                         "(ResidentTokenLoader; also reports host_us_per_step and kernel_us)")
    ap.add_argument("--kernel-sample", type=int, default=16,
                    help="resident: device events around the pack launch of every N-th step (kernel_us; 0 = none)")
    ap.add_argument("--plan", default="host", choices=["host", "device"],
                    help="resident: where a batch's order and pack plan are built. device: descriptor, plan and pack "
                         "are launches, with no host planning (in-order packing, fixed rows; the batch's counts "
                         "are device scalars)")
    ap.add_argument("--stream", action="store_true",
                    help="resident / zerocopy: the token stream format (ResidentTokenStreamLoader; with --path zerocopy "
                         "ZeroCopyTokenStreamLoader, whose gather_stream_pieces reads the plan's pieces from the "
                         "registered corpus over PCIe): --batch counts ROWS per rank per step, cut from the "
                         "concatenated shuffled documents; table, plan and pack are launches")
    ap.add_argument("--shuffle-rows", action="store_true",
                    help="with --stream: the epoch's rows in a shuffled order (shuffle_rows=True: the per-row plan "
                         "kernels in place of the contiguous plan)")
    ap.add_argument("--mix", default=None, metavar="R0,R1,...",
                    help="with --stream: repeats of equal parts of the corpus, e.g. 2,1,0.5 (TokenMix: the epoch's "
                         "document order is written by token_mix_order and read as an explicit index)")
    ap.add_argument("--fim", type=float, default=None, metavar="RATE",
                    help="with --stream: that share of the segments rearranged for fill-in-the-middle (TokenFIM, one "
                         "more launch per step); also reports, from the same job, the loader without it, run in turns "
                         "with it, and the token_fim kernel alone against a copy of the bytes it moves")
    ap.add_argument("--max-blocks", type=int, default=None,
                    help="zerocopy: grid cap of the gather kernel (0 = uncapped; default: the loader's)")
    ap.add_argument("--labels", action="store_true",
                    help="resident / zerocopy: the loader also delivers next-token labels (labels=True); the consumer "
                         "step is unchanged, so the rate against a run without the flag is the loader's cost")
    a = ap.parse_args(argv)
    zc = a.path in ("zerocopy", "resident")  # producer-free paths
    resident = a.path == "resident"
    if a.labels and not zc:
        ap.error("--labels needs --path resident or zerocopy (the producer path has no labels output)")
    if a.plan != "host" and not resident:
        ap.error("--plan device needs --path resident")
    if a.stream and (not zc or a.plan != "host" or a.mode != "pack"):
        ap.error("--stream needs --path resident or zerocopy, and is neither --plan device nor --mode pad")
    if a.shuffle_rows and not a.stream:
        ap.error("--shuffle-rows needs --stream")
    if a.mix and not a.stream:
        ap.error("--mix needs --stream")
    if a.fim is not None and not a.stream:
        ap.error("--fim needs --stream")
    if a.plan == "device" and a.mode == "pack":
        if a.pack_order == "ffd":
            ap.error("--plan device builds the in-order plan (--pack-order in_order) or, with one more kernel, the "
                     "first-fit-decreasing one (--pack-order ffd_device)")
        a.token_rows = "fixed"
    elif a.pack_order == "ffd_device" or a.max_rows is not None:
        ap.error("--pack-order ffd_device and --max-rows need --path resident --plan device --mode pack")

    import torch
    import torch.distributed as dist

    import ddl_amd
    from ddl_amd import ops
    from ddl_amd.models.tokens import SharedTokenSource, TokenBatchProducer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    name = f"ddl_amd_benchtok_{os.environ.get('MASTER_PORT', '0')}"
    src = None
    if int(os.environ.get("LOCAL_RANK", "0")) == 0:
        from ddl_amd.utils.numa import gpu_numa_node

        src = SharedTokenSource.synthetic(name, a.n_seqs, a.min_len, a.seq_len, seed=1, token_dtype=a.token_dtype)
        src.bind_to_node(gpu_numa_node(int(os.environ.get("LOCAL_RANK", "0"))))  # the producers' node
        from ddl_amd.models.datasets import SharedArraySource

        tb_seg = SharedArraySource(name + "_tb", 1, (1,), "int64", create=True)  # the wire dtype, for the node's ranks
        tb_seg.tensor().view(-1)[0] = src.token_bytes
    gb = a.batch * world
    try:
        with ddl_amd.start(n_producers=0 if zc else a.producers) as (env, conn):
            if env.world_size > 1:
                dist.barrier(group=env.control_group)
            if src is None:
                from ddl_amd.models.datasets import SharedArraySource

                # local rank 0 created the corpus; its wire dtype travels in the offsets segment's neighbour
                tb_view = SharedArraySource(name + "_tb", 1, (1,), "int64")  # held: its tensor maps the segment
                tb = int(tb_view.tensor().view(-1)[0])
                del tb_view
                t = SharedArraySource(name + "_tok", 0, (1,), torch.int32 if tb == 4 else torch.int16)
                o = SharedArraySource(name + "_off", a.n_seqs + 1, (1,), "int64")
                offs = o.tensor().view(-1).numpy()
                t.n = int(offs[-1])
                source = SharedTokenSource(t, o, int(np.diff(offs).max()))
            else:
                source = src
            n_epochs = (a.warmup + a.steps + a.idle_steps + a.warmup // 2) // (a.n_seqs // gb) + 2
            pack_order = a.pack_order if a.mode == "pack" else "in_order"
            if a.stream:
                mix = None
                if a.mix:  # equal parts of the corpus, by document index
                    repeat = [float(r) for r in a.mix.split(",")]
                    mix = ddl_amd.TokenMix([round(p * a.n_seqs / len(repeat)) for p in range(len(repeat) + 1)], repeat)
                fim = None
                if a.fim is not None:  # the sentinels past every id of the (at most 16-bit) synthetic vocabulary
                    fim = ddl_amd.TokenFIM(a.fim, prefix_id=65536, middle_id=65537, suffix_id=65538)

                def stream_loader(fim):
                    kw = dict(labels=a.labels, shuffle_rows=a.shuffle_rows, mix=mix, fim=fim)
                    if resident:
                        dl = ddl_amd.ResidentTokenStreamLoader(source, gb, a.seq_len, env, **kw)
                    else:
                        dl = ddl_amd.ZeroCopyTokenStreamLoader(source, gb, a.seq_len, env, max_blocks=a.max_blocks,
                                                               **kw)
                    dl.profile_every = a.kernel_sample
                    return dl

                dl = stream_loader(fim)
            elif resident:
                dl = ddl_amd.ResidentTokenLoader(source, gb, a.seq_len, a.mode, env, pack_order=pack_order,
                                                 token_rows=a.token_rows, n_epochs=n_epochs, plan=a.plan,
                                                 labels=a.labels, max_rows=a.max_rows)
                dl.profile_every = a.kernel_sample
            elif zc:
                dl = ddl_amd.ZeroCopyTokenLoader(source, gb, a.seq_len, a.mode, env, pack_order=pack_order,
                                                 token_rows=a.token_rows, max_blocks=a.max_blocks, n_epochs=n_epochs,
                                                 labels=a.labels)
            else:
                producer = TokenBatchProducer(source, gb, a.seq_len, a.mode, pack_order=pack_order,
                                              batches_per_window=a.batches_per_window, host_threads=a.host_threads)
                dispatch = False if a.dispatch == "python" else a.dispatch
                dl = ddl_amd.DistributedDataLoader(producer, a.batch, conn, n_epochs, env=env, auto_mark=True,
                                                   output=ddl_amd.OutputSpec(collate="tokens",
                                                                             token_rows=a.token_rows),
                                                   staging=ddl_amd.StagingSpec(n_slots=a.slots,
                                                                               native_dispatch=dispatch),
                                                   order=ddl_amd.OrderSpec(mode="indexed"))
            dev = torch.device(env.device)
            acc = ops.ChecksumAccumulator(dev)  # one streaming launch per batch

            def sync():  # the CPU rehearsal (DDL_DEVICE=cpu) has nothing to synchronise
                if dev.type == "cuda":
                    torch.cuda.synchronize(dev)

            def gen():
                while True:
                    yield from dl

            it = gen()
            real = 0
            for _ in range(a.warmup):
                b = next(it)
                acc.add(b["input_ids"])
            sync()
            if env.world_size > 1:
                dist.barrier(group=env.control_group)
            t0 = time.perf_counter()
            rows = delivered = 0
            dev_counts = None  # plan="device": the counts are device scalars, summed there and read once
            for _ in range(a.steps):
                b = next(it)
                acc.add(b["input_ids"])
                delivered += b["input_ids"].numel()  # positions written and handed over, padding included
                if torch.is_tensor(b["n_tokens"]):
                    if dev_counts is None:
                        dev_counts = torch.zeros(2, dtype=torch.int64, device=b["n_tokens"].device)
                    dev_counts[0].add_(b["n_tokens"])
                    if "n_rows" in b:
                        dev_counts[1].add_(b["n_rows"])
                    else:
                        rows += b["input_ids"].shape[0]
                    continue
                rows += b.get("n_rows", b["input_ids"].shape[0])
                real += b["n_tokens"]  # counted from the delivered batches (producer tag), not estimated
            sync()
            dt = time.perf_counter() - t0
            if dev_counts is not None:
                real += int(dev_counts[0])
                rows += int(dev_counts[1])
            st = dl.stats()
            ffd_kernel_us = None
            if pack_order == "ffd_device" and dev.type == "cuda":
                # the new launch alone, between device events, over this rank's first batches of epoch 0
                offs_dev = source.offsets.tensor().view(-1).to(dev)
                evs = []
                for g in range(32):  # the epoch's batches, round and round
                    g %= a.n_seqs // gb
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ops.ffd_index_device(offs_dev, perm=dl.order.perm(0), base=g * gb + env.rank * a.batch,
                                         count=a.batch, seq_len=a.seq_len)
                    e1.record()
                    evs.append((e0, e1))
                sync()
                ffd_kernel_us = round(1e3 * sum(x.elapsed_time(y) for x, y in evs[4:]) / max(1, len(evs) - 4), 1)
            timed = resident or a.stream  # the loaders with a launch frame
            timing = dl.timing() if timed else None  # of the measured phase and its warm-up
            if timed:
                dl.profile_every = 0
            if env.world_size > 1:
                t = torch.tensor([dt], dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=env.control_group)
                dt = float(t.item())
            idle = None
            if a.idle_steps and dev.type == "cuda":
                # phase 2: GPU idle % behind a fixed-cost bf16 token train step (BASELINE config 4)
                from ddl_amd.models.trainstep import TokenTrainStep
                from ddl_amd.utils.tracing import ComputeIdleMeter

                step = TokenTrainStep(dev, seq_len=a.seq_len, dim=a.model_dim, depth=a.model_depth)
                for _ in range(max(1, a.warmup // 2)):
                    step(next(it))
                meter = ComputeIdleMeter()
                sync()
                t2 = time.perf_counter()
                for _ in range(a.idle_steps):
                    b = next(it)
                    meter.step_begin()
                    step(b)
                    meter.step_end()
                sync()
                t3 = time.perf_counter()
                idle = meter.result()
                idle["train_sequences_per_s"] = a.idle_steps * a.batch * env.world_size / (t3 - t2)
                if env.world_size > 1:
                    t = torch.tensor([idle["gpu_idle_pct"]], dtype=torch.float64)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=env.control_group)
                    idle["gpu_idle_pct"] = float(t.item())
            toks = source.offsets.tensor().view(-1).numpy()
            mean_len = float(np.diff(toks).mean())
            est_tokens = a.steps * a.batch * mean_len * env.world_size
            real_tokens = real
            if env.world_size > 1:
                t = torch.tensor([real], dtype=torch.float64)
                dist.all_reduce(t, group=env.control_group)
                real_tokens = float(t.item())
            bpw = None if zc else dl.batches_per_window[0]
            if env.world_size > 1:
                t = torch.tensor([delivered], dtype=torch.float64)
                dist.all_reduce(t, group=env.control_group)
                delivered = float(t.item())
            dl.close()
            fim_report = None
            if a.stream and a.fim is not None and dev.type == "cuda":
                fim_report = _fim_report(a, stream_loader, fim, dev)
            if env.rank == 0:
                if resident:
                    per_path = {"path": "resident", "handoff": st["handoff"], "host_waits": st["host_waits"],
                                "host_us_per_step": round(timing["host_us_per_step"], 1),
                                "kernel_us": None if timing["kernel_us"] is None else round(timing["kernel_us"], 1),
                                "kernel_samples": timing["kernel_samples"],
                                "load_s": round(st["load_s"], 3), "load_gbps": round(st["load_gbps"], 2),
                                "replica_shared": st["replica_shared"], "plan": "stream" if a.stream else a.plan}
                    if pack_order == "ffd_device" or a.max_rows is not None:
                        per_path.update(max_rows=a.max_rows, ffd_kernel_us=ffd_kernel_us,
                                        static_rows=int(delivered // (a.steps * a.seq_len * env.world_size)))
                    if a.stream:
                        per_path.update(format="stream", max_segments=st["max_segments"],
                                        tables_built=st["tables_built"], shuffle_rows=st["shuffle_rows"],
                                        mix=a.mix, mix_parts=st["mix_parts"], mix_documents=st["mix_documents"],
                                        orders_built=st["orders_built"],
                                        epoch_prep_us=None if timing["epoch_prep_us"] is None
                                        else round(timing["epoch_prep_us"], 1),
                                        epoch_prep_samples=timing["epoch_prep_samples"])
                elif zc:
                    per_path = {"path": "zerocopy", "max_blocks": st["max_blocks"], "host_waits": st["host_waits"],
                                "prefault_s": round(st["prefault_s"], 3)}
                    if a.stream:
                        per_path.update(plan="stream", format="stream", handoff=st["handoff"],
                                        host_us_per_step=round(timing["host_us_per_step"], 1),
                                        kernel_us=None if timing["kernel_us"] is None
                                        else round(timing["kernel_us"], 1),
                                        kernel_samples=timing["kernel_samples"], hbm_bytes=st["hbm_bytes"],
                                        max_segments=st["max_segments"], tables_built=st["tables_built"],
                                        shuffle_rows=st["shuffle_rows"], mix=a.mix, mix_parts=st["mix_parts"],
                                        mix_documents=st["mix_documents"], orders_built=st["orders_built"],
                                        epoch_prep_us=None if timing["epoch_prep_us"] is None
                                        else round(timing["epoch_prep_us"], 1),
                                        epoch_prep_samples=timing["epoch_prep_samples"])
                else:
                    per_path = {
                        "producers": a.producers, "host_threads": a.host_threads, "slots": a.slots,
                        "batches_per_window": bpw, "dispatch": a.dispatch,
                        "dispatch_mode": (st.get("native_dispatch") or {}).get("mode"),
                        "consumer_wait_s": round(st["consumer_wait_s"], 3),
                        "stager_wait_producer_s": round(st.get("stager_wait_producer_s", 0.0), 3),
                        # per producer: rounds, mean fill and mean slot-wait per round (us) -- where the feed goes
                        "producers_rounds_fill_wait_us": [
                            (p["rounds"], round(p["fill_ns_total"] / max(1, p["rounds"]) / 1e3, 1),
                             round(p["wait_ns_total"] / max(1, p["rounds"]) / 1e3, 1))
                            for p in st.get("producers", [])]}
                res = {
                    "metric": "tokens/s fed to GPU (seq_len 4096, on-device pad/pack)", "mode": a.mode,
                    "value": round(real_tokens / dt, 1), "unit": "tokens/s (real tokens delivered)",
                    "delivered_tokens_per_s": round(delivered / dt, 1),
                    "delivered_density": round(real_tokens / max(delivered, 1), 4),
                    "value_est_from_mean_len": round(est_tokens / dt, 1),
                    "sequences_per_s": round(a.steps * a.batch * env.world_size / dt, 1),
                    "packed_rows_per_step": round(rows / a.steps, 2),
                    "pack_order": a.pack_order if a.mode == "pack" else None,
                    "row_density": round(real / max(rows * a.seq_len, 1), 3),
                    "row_density_est": round(a.batch * mean_len / (rows / a.steps) / a.seq_len, 3),
                    "n_gpus": env.world_size,
                    "steps": a.steps, "ms_per_step": round(1000 * dt / a.steps, 3), "batch_seqs": a.batch,
                    "token_rows": a.token_rows, **({"labels": True} if a.labels else {}),
                    "mean_len": round(mean_len, 1),
                    "token_wire_dtype": "uint16" if source.token_bytes == 2 else "int32",
                    "h2d_token_gbps": round(real_tokens * source.token_bytes / dt / 1e9, 2),
                    **per_path, **({"fim": fim_report} if fim_report is not None else {}),
                    "gpu_idle_pct": None if idle is None else round(idle["gpu_idle_pct"], 3),
                    "train_step": None if idle is None else {
                        "model": f"TokenMLP dim={a.model_dim} depth={a.model_depth} fwd+bwd+SGD bf16",
                        "sequences_per_s": round(idle["train_sequences_per_s"], 1),
                        "busy_ms": round(idle["busy_ms"], 3), "wall_ms": round(idle["wall_ms"], 3)}}
                print(json.dumps(res), flush=True)
    finally:
        if src is not None:
            src.close()
            tb_seg.close()


if __name__ == "__main__":
    sys.exit(main())
