#!/usr/bin/env python3
"""Per-kernel throughput of the gfx950 loader kernels at production shapes.

Each kernel is timed with HIP events over many launches and reported as
effective HBM GB/s (bytes read + written) against two denominators: the
8 TB/s HBM3E spec (``pct_of_spec``) and a roofline MEASURED first on the same
box: the best of a 1 GiB device-to-device ``copy_`` and a plain streaming-copy
kernel (``pct_of_d2d``: read + write bytes over its time). A kernel timed in a
loop over one batch-sized buffer (77 MB in, 77 MB out) is partly served by the
256 MB Infinity Cache and can exceed that HBM roofline; the same streaming copy
at that working set is printed as a reference. No child processes, no producers: safe to run under
``rocprofv3 --pmc``.
"""

import json
import sys

import numpy as np
import torch

from ddl_amd import ops
from ddl_amd.permutation import FeistelPermutation


def bench(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


HBM_SPEC_BPS = 8.0e12
D2D_BPS = None  # measured in main()


def report(name, t, bytes_moved, **kw):
    bps = bytes_moved / t
    print(json.dumps({"kernel": name, "us": round(t * 1e6, 2), "GBps": round(bps / 1e9, 1),
                      "pct_of_spec": round(100 * bps / HBM_SPEC_BPS, 1),
                      "pct_of_d2d": round(100 * bps / D2D_BPS, 1) if D2D_BPS else None, **kw}), flush=True)


def measure_d2d() -> float:
    """Measured HBM roofline: the best (bytes read + written) / s of two 1 GiB device-to-device copies,
    the runtime's ``copy_`` (hipMemcpy D2D) and a plain 16 B-per-lane streaming copy kernel
    (``stream_copy``, grid sized 2..16 blocks per CU)."""
    global D2D_BPS
    from ddl_amd import _native

    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    best = {}
    t = bench(lambda: b.copy_(a), reps=20)
    best["copy_ (hipMemcpy D2D)"] = t
    hip = _native.hip()
    st = torch.cuda.current_stream().cuda_stream
    for bpc in (2, 4, 8, 16):
        t = bench(lambda: hip.stream_copy(a.data_ptr(), b.data_ptr(), a.numel(), 256 * bpc, st), reps=20)
        best[f"stream_copy {bpc}x256 blocks"] = t
    # one pass: every thread moves 4 x 16 B once (no grid-stride loop); the fastest copy shape measured at
    # 4 GiB by benchmarks/hbm_ceilings.hip (5.69 TB/s), which also gives the read-only / write-only ceilings
    one_shot = a.numel() // 16 // (256 * 4)
    t = bench(lambda: hip.stream_copy(a.data_ptr(), b.data_ptr(), a.numel(), one_shot, st), reps=20)
    best["stream_copy one pass"] = t
    for name, t in best.items():
        bps = 2 * a.numel() / t
        print(json.dumps({"kernel": f"roofline: {name} 1GiB", "us": round(t * 1e6, 2), "GBps": round(bps / 1e9, 1),
                          "pct_of_spec": round(100 * bps / HBM_SPEC_BPS, 1)}), flush=True)
    D2D_BPS = 2 * a.numel() / min(best.values())
    # the same copy at the gathers' working set (77 MB in + 77 MB out): it fits the 256 MB Infinity Cache
    # (MALL) when repeated, which is why kernels on batch-sized buffers can exceed the 1 GiB HBM roofline
    ws = 256 * 3 * 224 * 224 * 2
    for bpc in (2, 4):
        t = bench(lambda: hip.stream_copy(a.data_ptr(), b.data_ptr(), ws, 256 * bpc, st), reps=50)
        print(json.dumps({"kernel": f"reference: stream_copy {bpc}x256 blocks 77MB (batch working set)",
                          "us": round(t * 1e6, 2), "GBps": round(2 * ws / t / 1e9, 1),
                          "pct_of_spec": round(100 * 2 * ws / t / HBM_SPEC_BPS, 1),
                          "pct_of_d2d": round(100 * 2 * ws / t / D2D_BPS, 1)}), flush=True)
    return D2D_BPS


def main():
    dev = torch.device("cuda", 0)
    measure_d2d()
    B, C, H, W = 256, 3, 224, 224
    n = 2048
    win_bf16 = torch.randn(n, C, H, W, device=dev).to(torch.bfloat16)
    win_u8 = torch.randint(0, 256, (n, C, H, W), dtype=torch.uint8, device=dev)
    win_hwc = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, device=dev)
    p = FeistelPermutation(n, 1, 2)
    out_bf16 = torch.empty(B, C, H, W, dtype=torch.bfloat16, device=dev)
    img = C * H * W
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    sc = [1 / (255 * s_) for s_ in std]
    bi = [-m / s_ for m, s_ in zip(mean, std)]

    t = bench(lambda: ops.gather_rows(win_bf16, perm=p, base=0, n_rows=B, out=out_bf16))
    report("permute_gather bf16->bf16", t, 2 * B * img * 2, rows=B, row_bytes=img * 2)
    t = bench(lambda: ops.gather_rows(win_u8, perm=p, base=0, n_rows=B, out=out_bf16, scale=sc, bias=bi,
                                      plane=H * W))
    report("permute_gather u8->bf16 normalise", t, B * img * 3, rows=B)
    t = bench(lambda: ops.collate_hwc_to_chw(win_hwc, perm=p, base=0, n_rows=B, out=out_bf16, mean=mean, std=std))
    report("collate HWC u8 -> CHW bf16 normalise", t, B * img * 3, rows=B)
    f32 = torch.randn(B, img, device=dev)
    t = bench(lambda: ops.cast(f32, torch.bfloat16))
    report("cast f32->bf16", t, B * img * 6)
    idx = torch.from_numpy(p(np.arange(B))).to(dev)
    t = bench(lambda: ops.scatter_rows(win_bf16.view(n, -1), out_bf16.view(B, -1), idx))
    report("scatter_rows bf16", t, 2 * B * img * 2)
    t = bench(lambda: ops.checksum(out_bf16))
    report("checksum (reduce)", t, B * img * 2)
    cacc = ops.ChecksumAccumulator(dev)
    t = bench(lambda: cacc.add(out_bf16))
    report("checksum accumulate (streaming consumer)", t, B * img * 2)
    t = bench(lambda: ops.feistel_indices(FeistelPermutation(1 << 24, 3, 3), 0, 1 << 24, device=dev), reps=10)
    report("feistel_indices 16M", t, (1 << 24) * 8)
    # augmentation: RandomResizedCrop 256x320 u8 -> 224x224 bf16 (+ flip + normalise), CHW and HWC sources
    for layout in ("chw", "hwc"):
        shp = (1024, 3, 256, 320) if layout == "chw" else (1024, 256, 320, 3)
        raw = torch.randint(0, 255, shp, dtype=torch.uint8, device=dev)
        p1k = FeistelPermutation(1024, 1, 3)
        t = bench(lambda: ops.random_resized_crop(raw, perm=p1k, base=0, n_rows=B, size=(224, 224), seed=1,
                                                  layout=layout, mean=[0.5] * 3, std=[0.25] * 3))
        report(f"random_resized_crop {layout} u8 256x320 -> bf16 224x224", t, B * img * 2)
    # pointwise (reference CI shape): 100,520 x 9 f32 window, 4096-row batch split (3,5,1)
    pw = torch.randn(100_520, 9, device=dev)
    pp = FeistelPermutation(100_520, 5, 5)
    t = bench(lambda: ops.split_columns(pw, (3, 5, 1), perm=pp, base=0, n_rows=4096))
    report("split_columns 4096x(3,5,1) f32", t, 2 * 4096 * 36)
    # whole-window dispatch: the window's 24 batches in one launch (same kernel, 24x the rows)
    t = bench(lambda: ops.split_columns(pw, (3, 5, 1), perm=pp, base=0, n_rows=24 * 4096))
    report("split_columns 24x4096x(3,5,1) f32 (one launch per window)", t, 2 * 24 * 4096 * 36)
    # resident exchange bucketing (W=8, global batch 2048): send list + receive map, one workgroup each
    from ddl_amd import _native

    hip = _native.hip()
    pr = FeistelPermutation(1 << 20, 7, 1)
    S, W, GB, LB, rank = (1 << 20) // 8, 8, 2048, 256, 1
    send_idx = torch.empty(GB, dtype=torch.int64, device=dev)
    inv_idx = torch.empty(LB, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    send_c, recv_c = _native.runtime().owner_counts(pr.keys, pr.half_bits, pr.n, 0, GB, LB, S, W, rank)
    t = bench(lambda: hip.bucket_send(pr.keys, pr.n, pr.half_bits, 0, GB, S, S * rank, rank, W,
                                      send_idx.data_ptr(), st))
    report("bucket_send W=8 GB=2048", t, GB * 8, sent=sum(send_c))
    offs = [0]
    for c in recv_c[:-1]:
        offs.append(offs[-1] + c)
    t = bench(lambda: hip.bucket_recv(pr.keys, pr.n, pr.half_bits, rank * LB, LB, S, W, offs,
                                      inv_idx.data_ptr(), st))
    report("bucket_recv W=8 slice 256", t, LB * 8)
    grp = [pw[:, :3].contiguous(), pw[:, 3:8].contiguous(), pw[:, 8:].contiguous()]
    t = bench(lambda: ops.pack_columns(grp))
    report("pack_columns window 100520x(3,5,1) f32", t, 2 * 100_520 * 36)
    t = bench(lambda: ops.pack_columns(grp, perm=pp, base=0, n_rows=4096, out_dtype=torch.bfloat16))
    report("pack_columns 4096 gather+bf16", t, 4096 * 36 + 4096 * 18)
    # tokens: 64 sequences, mean 2k, seq_len 4096 pack + pad
    rng = np.random.default_rng(0)
    lens = rng.integers(256, 4097, size=64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = torch.from_numpy(rng.integers(0, 50000, size=int(offs[-1])).astype(np.int32)).to(dev)
    offs_d = torch.from_numpy(offs).to(dev)
    t = bench(lambda: ops.pad_tokens(toks, offs_d, 4096))
    report("pad_tokens 64x4096", t, toks.numel() * 4 + 64 * 4096 * (4 + 1 + 8))
    t = bench(lambda: ops.pack_tokens(toks, offs, 4096), reps=20)
    report("pack_tokens 64 seqs (incl. host plan)", t, toks.numel() * (4 + 4 + 1 + 8 + 4))
    # the plan on the device: plan kernel + pack kernel reading the row count from device memory (no host
    # round trip; static shapes), output rows = pack_capacity
    t = bench(lambda: ops.pack_tokens_device(toks, offs_d, 4096), reps=20)
    report("pack_tokens 64 seqs (device plan, 2 launches)", t, toks.numel() * (4 + 4 + 1 + 8 + 4))
    lens2 = rng.integers(1, 4097, size=2048)
    offs2 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)).to(dev)
    toks2 = torch.from_numpy(rng.integers(0, 50000, size=int(lens2.sum())).astype(np.int32)).to(dev)
    t = bench(lambda: ops.pack_tokens_device(toks2, offs2, 4096), reps=20)
    report("pack_tokens 2048 seqs (device plan, 2 launches)", t, toks2.numel() * (4 + 4 + 1 + 8 + 4))
    t = bench(lambda: ops.pack_tokens(toks2, offs2.cpu().numpy(), 4096), reps=10)
    report("pack_tokens 2048 seqs (incl. host plan)", t, toks2.numel() * (4 + 4 + 1 + 8 + 4))
    # the same two launches captured in a HIP graph: device time only (no Python / allocator on the host)
    for name, (tk, of) in (("64", (toks, offs_d)), ("2048", (toks2, offs2))):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.pack_tokens_device(tk, of, 4096)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.pack_tokens_device(tk, of, 4096)
        t = bench(g.replay, reps=20)
        report(f"pack_tokens {name} seqs (device plan, graph replay)", t, tk.numel() * (4 + 4 + 1 + 8 + 4))
    x = torch.randn(1_000_000, 9, device=dev)
    t = bench(lambda: ops.column_stats(x), reps=20)
    report("column_stats 1Mx9", t, x.numel() * 4)
    del win_bf16, win_u8, win_hwc, raw, pw, x
    out_of_cache(dev)
    tokens_indexed(dev)


def rotating(fns, reps=48):
    """Time a list of calls issued round-robin (each touches its own buffers), per call."""
    i = [0]

    def one():
        fns[i[0] % len(fns)]()
        i[0] += 1

    return bench(one, reps=reps)


def out_of_cache(dev) -> None:
    """The gather / cast / scatter kernels on working sets far beyond the 256 MB MALL: 1024-row batches
    from an 8192-image window (2.5 GB bf16 / 1.2 GB uint8), 4 output buffers used round-robin, so every
    call reads and writes memory the previous calls did not touch (>= 1.2 GB in flight per rotation).
    These are the numbers to hold against the 1 GiB D2D roofline (``pct_of_d2d``)."""
    B, C, H, W, n = 1024, 3, 224, 224, 8192
    img = C * H * W
    p = FeistelPermutation(n, 1, 2)
    win = torch.empty(n, C, H, W, dtype=torch.bfloat16, device=dev).normal_()
    outs = [torch.empty(B, C, H, W, dtype=torch.bfloat16, device=dev) for _ in range(4)]
    fns = [lambda o=o, k=k: ops.gather_rows(win, perm=p, base=k * B, n_rows=B, out=o) for k, o in enumerate(outs)]
    report("OOC permute_gather bf16->bf16 1024 rows (rotating)", rotating(fns), 2 * B * img * 2, rows=B)
    idxs = [torch.from_numpy(p(np.arange(k * B, (k + 1) * B))).to(dev) for k in range(4)]
    fns = [lambda o=o, ix=ix: ops.scatter_rows(win.view(n, -1), o.view(B, -1), ix) for o, ix in zip(outs, idxs)]
    report("OOC scatter_rows bf16 1024 rows (rotating)", rotating(fns), 2 * B * img * 2, rows=B)
    del win
    win8 = torch.randint(0, 256, (n, C, H, W), dtype=torch.uint8, device=dev)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    sc = [1 / (255 * s_) for s_ in std]
    bi = [-m / s_ for m, s_ in zip(mean, std)]
    fns = [lambda o=o, k=k: ops.gather_rows(win8, perm=p, base=k * B, n_rows=B, out=o, scale=sc, bias=bi,
                                            plane=H * W) for k, o in enumerate(outs)]
    report("OOC permute_gather u8->bf16 normalise 1024 rows (rotating)", rotating(fns), B * img * 3, rows=B)
    del win8
    f32s = [torch.empty(B, img, device=dev).normal_() for _ in range(2)]
    fns = [lambda f=f, o=o: ops.gather_rows(f, out=o.view(B, img)) for f, o in zip(f32s * 2, outs)]
    report("OOC cast f32->bf16 1024 rows (rotating)", rotating(fns), B * img * 6, rows=B)


COPY_CEILING_BPS = 5.69e12  # one-pass HBM copy ceiling (docs/PERFORMANCE.md), read + write bytes


def tokens_indexed(dev, repeats=5) -> None:
    """The fused indexed pad/pack kernel against gather_ragged (HBM source) + pad_pack_tokens on the same input:
    a uint16 corpus far beyond the 256 MB MALL (131072 sequences, lengths uniform in [256, 4096]: ~570 MB), 2048
    sequences per batch, seq_len 4096, pack. 4 batches (own indices, own outputs: ~300 MB written per rotation)
    are issued round-robin at launcher level, descriptors already on the device, so the times are device times.
    One JSON line per repeat and a summary; the outputs of the two routes are compared first."""
    from ddl_amd import _native
    from ddl_amd.ops.kernels import carve_token_outputs, segment_sources, token_output_bytes

    hip = _native.hip()
    rng = np.random.default_rng(0)
    n_src, B, S, rot = 131072, 2048, 4096, 4
    lens = rng.integers(256, 4097, size=n_src)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    corpus = torch.randint(0, 32768, (int(offs[-1]),), dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cases = []
    for _ in range(rot):
        idx = rng.choice(n_src, size=B, replace=False).astype(np.int64)
        start = np.ascontiguousarray(offs[idx])
        dofs = np.concatenate([[0], np.cumsum(offs[idx + 1] - offs[idx])]).astype(np.int64)
        rs, re_, so = ops.pack_plan(dofs, S)
        R, n_seg, T = len(rs), len(so) - 1, int(dofs[-1])
        seg_src = np.ascontiguousarray(segment_sources(start, dofs, so, n_seg))
        tiles = np.zeros(B + 1, dtype=np.int32)
        n_tiles = hip.ragged_tile_plan(corpus.data_ptr(), start.ctypes.data, dofs.ctypes.data, B, 2, tiles.ctypes.data)
        d = {k: torch.from_numpy(v).to(dev) for k, v in dict(start=start, dofs=dofs, rs=rs, re=re_, so=so,
                                                             seg_src=seg_src, tiles=tiles).items()}
        flat = torch.empty(T, dtype=torch.int16, device=dev)
        outs = [carve_token_outputs(torch.empty(token_output_bytes(R, S, n_seg), dtype=torch.uint8, device=dev), R, S,
                                    n_seg) for _ in range(2)]
        cases.append((d, flat, outs, R, n_seg, T, n_tiles))

    def out_kw(o):
        ids, mask, pos, seg, cu = o
        return dict(out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(), pos_is_i64=True,
                    segment_ids=seg.data_ptr(), cu_seqlens_out=cu.data_ptr())

    def fused(c, o=0):
        d, _, outs, R, n_seg, _, _ = c
        hip.pad_pack_tokens_indexed(corpus=corpus.data_ptr(), corpus_elems=corpus.numel(),
                                    src_start=d["start"].data_ptr(), seg_src=d["seg_src"].data_ptr(), offsets=0,
                                    row_start=d["rs"].data_ptr(), row_end=d["re"].data_ptr(),
                                    seg_offsets=d["so"].data_ptr(), n_seg=n_seg, rows=R, seq_len=S, pad_id=0, mode=1,
                                    stream=stream, tok16=True, **out_kw(outs[o]))

    def gather(c):
        d, flat, _, _, _, _, n_tiles = c
        hip.gather_ragged(dst=flat.data_ptr(), src=corpus.data_ptr(), src_start=d["start"].data_ptr(),
                          dst_offsets=d["dofs"].data_ptr(), tile_start=d["tiles"].data_ptr(), n=B, n_tiles=n_tiles,
                          elem_bytes=2, max_blocks=0, stream=stream)

    def pack(c, o=1):
        d, flat, outs, R, n_seg, _, _ = c
        hip.pad_pack_tokens(tokens=flat.data_ptr(), offsets=0, row_start=d["rs"].data_ptr(),
                            row_end=d["re"].data_ptr(), seg_offsets=d["so"].data_ptr(), n_seg=n_seg, rows=R, seq_len=S,
                            pad_id=0, mode=1, stream=stream, tok16=True, **out_kw(outs[o]))

    def both(c):
        gather(c)
        pack(c)

    for c in cases:  # the two routes write the same bytes
        fused(c)
        both(c)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(c[2][0], c[2][1])), "fused and two-kernel outputs differ"
    R_mean = float(np.mean([c[3] for c in cases]))
    T_mean = float(np.mean([c[5] for c in cases]))
    wr = 17 * R_mean * S  # ids 4 + i64 positions 8 + segment ids 4 + mask 1 per output position
    bytes_fused, bytes_two = 2 * T_mean + wr, 2 * T_mean + 2 * T_mean + 2 * T_mean + wr
    runs = []
    for r in range(repeats):
        t = {name: rotating([lambda c=c, fn=fn: fn(c) for c in cases])
             for name, fn in (("fused", fused), ("gather_ragged", gather), ("pad_pack_tokens", pack),
                              ("two_kernels", both))}
        runs.append(t)
        print(json.dumps({"kernel": "tokens_indexed vs gather_ragged + pad_pack_tokens", "repeat": r,
                          **{k + "_us": round(v * 1e6, 2) for k, v in t.items()},
                          "sum_us": round((t["gather_ragged"] + t["pad_pack_tokens"]) * 1e6, 2)}), flush=True)
    med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
    sums = [t["gather_ragged"] + t["pad_pack_tokens"] for t in runs]
    print(json.dumps({
        "kernel": "tokens_indexed summary", "sequences": B, "seq_len": S, "token_dtype": "uint16",
        "corpus_mb": round(corpus.numel() * 2 / 1e6, 1), "rows": R_mean, "tokens": T_mean, "repeats": repeats,
        "fused_us_median": round(med["fused"] * 1e6, 2),
        "fused_us_min_max": [round(min(t["fused"] for t in runs) * 1e6, 2), round(max(t["fused"] for t in runs) * 1e6, 2)],
        "sum_us_median": round(float(np.median(sums)) * 1e6, 2),
        "sum_us_min_max": [round(min(sums) * 1e6, 2), round(max(sums) * 1e6, 2)],
        "two_kernels_back_to_back_us_median": round(med["two_kernels"] * 1e6, 2),
        "fused_bytes": int(bytes_fused), "two_kernel_bytes": int(bytes_two),
        "fused_GBps": round(bytes_fused / med["fused"] / 1e9, 1),
        "two_kernel_GBps": round(bytes_two / float(np.median(sums)) / 1e9, 1),
        "fused_pct_of_copy_ceiling": round(100 * bytes_fused / med["fused"] / COPY_CEILING_BPS, 1),
        "fused_tokens_per_s": round(T_mean / med["fused"], 1)}), flush=True)


def tokens_plan(dev, repeats=5) -> None:
    """The device-built batch plan at the ``tokens_indexed`` shape (uint16 corpus of 131072 sequences, 2048
    sequences per batch, seq_len 4096, pack, fixed rows): ``token_batch_descriptor`` + ``pack_plan_device`` -- one
    workgroup each, added to every ``plan="device"`` step -- and the pack kernel reading the plan's counts from
    device memory, against the same kernel under the host plan (descriptor already on the device). 4 batches
    (positions of one Feistel order, own plan arrays, own outputs) are issued round-robin at launcher level, so
    the times are device times. The outputs of the two routes are compared first."""
    from ddl_amd import _native
    from ddl_amd.ops.kernels import (_index_kw, carve_token_outputs, device_batch_bytes, device_plan_bytes,
                                     launch_device_plan, segment_sources, token_output_bytes)

    hip = _native.hip()
    rng = np.random.default_rng(0)
    n_src, B, S, rot = 131072, 2048, 4096, 4
    lens = rng.integers(256, 4097, size=n_src)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    corpus = torch.randint(0, 32768, (int(offs[-1]),), dtype=torch.int16, device=dev)
    coffs = torch.from_numpy(offs).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    perm = FeistelPermutation(n_src, 3, 1)
    M = R = B  # the loader's capacities: layout.max_segments = B * ceil(max_len / S)
    plan_b = device_plan_bytes(B, M, R)
    cases = []
    for k in range(rot):
        idx = perm(np.arange(k * B, (k + 1) * B, dtype=np.int64))
        start = np.ascontiguousarray(offs[idx])
        dofs = np.concatenate([[0], np.cumsum(offs[idx + 1] - offs[idx])]).astype(np.int64)
        rs, re_, so = ops.pack_plan(dofs, S)
        n_rows, n_seg, T = len(rs), len(so) - 1, int(dofs[-1])
        seg_src = np.ascontiguousarray(segment_sources(start, dofs, so, n_seg))
        d = {k_: torch.from_numpy(v).to(dev) for k_, v in dict(start=start, rs=rs, re=re_, so=so,
                                                               seg_src=seg_src).items()}
        host_out = carve_token_outputs(torch.empty(token_output_bytes(R, S, n_seg), dtype=torch.uint8, device=dev),
                                       R, S, n_seg)
        plan = torch.empty(plan_b, dtype=torch.uint8, device=dev)
        whole = torch.empty(device_batch_bytes(R, S, M), dtype=torch.uint8, device=dev)
        cases.append(dict(d=d, host_out=host_out, plan=plan, whole=whole, n_rows=n_rows, n_seg=n_seg, T=T,
                          sel=_index_kw(None, perm, k * B)))

    def device_route(c):
        return launch_device_plan(c["plan"].data_ptr(), c["whole"], corpus_ptr=corpus.data_ptr(),
                                  corpus_elems=corpus.numel(), tok16=True, corpus_offsets_ptr=coffs.data_ptr(),
                                  n_corpus=n_src, selector=c["sel"], n=B, seq_len=S, pad_id=0, pack=True, max_segs=M,
                                  max_rows=R, stream=stream)

    def host_pack(c):
        d = c["d"]
        ids, mask, pos, seg, cu = c["host_out"]
        hip.pad_pack_tokens_indexed(corpus=corpus.data_ptr(), corpus_elems=corpus.numel(),
                                    src_start=d["start"].data_ptr(), seg_src=d["seg_src"].data_ptr(), offsets=0,
                                    row_start=d["rs"].data_ptr(), row_end=d["re"].data_ptr(),
                                    seg_offsets=d["so"].data_ptr(), n_seg=c["n_seg"], rows=c["n_rows"], seq_len=S,
                                    pad_id=0, mode=1, stream=stream, tok16=True, fill_rows=R,
                                    out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(),
                                    pos_is_i64=True, segment_ids=seg.data_ptr(), cu_seqlens_out=cu.data_ptr())

    for c in cases:  # the two routes write the same bytes
        r = device_route(c)
        host_pack(c)
        torch.cuda.synchronize()
        ids, mask, pos, seg, cu = c["host_out"]
        assert r["counts"].tolist()[:3] == [c["n_rows"], c["n_seg"], c["T"]], "device and host plans differ"
        assert all(torch.equal(a, b) for a, b in zip((r["input_ids"], r["attention_mask"], r["position_ids"],
                                                      r["segment_ids"]), (ids, mask, pos, seg))), "outputs differ"
        assert torch.equal(r["cu_seqlens"][:c["n_seg"] + 1], cu)
        assert bool((r["cu_seqlens"][c["n_seg"]:] == c["T"]).all())
        # the three launches of the device route, one by one, on this batch's own arrays
        p, n = c["plan"].data_ptr(), B
        a16 = lambda v: -(-v // 16) * 16  # noqa: E731
        o_off = p + a16(8 * n)
        o_ss = o_off + a16(8 * (n + 1))
        o_so = o_ss + a16(8 * M)
        o_rs = o_so + a16(8 * (M + 1))
        o_re = o_rs + a16(8 * R)
        o_scr = o_re + a16(8 * R)
        cp = r["counts"].data_ptr()
        c["descriptor"] = lambda p=p, o_off=o_off, o_ss=o_ss, cp=cp, sel=c["sel"]: hip.token_batch_descriptor(
            corpus_offsets=coffs.data_ptr(), n_corpus=n_src, n=B, seq_len=S, max_segs=M, src_start=p, offsets=o_off,
            seg_src=o_ss, counts=cp, pad_counts=False, stream=stream, **sel)
        c["plan_kernel"] = lambda o_off=o_off, o_so=o_so, o_rs=o_rs, o_re=o_re, o_scr=o_scr, cp=cp: (
            hip.pack_plan_device)(
            offsets=o_off, n=B, seq_len=S, max_segs=M, max_rows=R, seg_offsets=o_so, row_start=o_rs, row_end=o_re,
            counts=cp, scratch=o_scr, stream=stream)
        c["device_pack"] = lambda p=p, o_ss=o_ss, o_so=o_so, o_rs=o_rs, o_re=o_re, cp=cp, r=r: (
            hip.pad_pack_tokens_indexed)(
            corpus=corpus.data_ptr(), corpus_elems=corpus.numel(), src_start=p, seg_src=o_ss, offsets=0,
            row_start=o_rs, row_end=o_re, seg_offsets=o_so, n_seg=0, rows=0, seq_len=S, pad_id=0, mode=1,
            stream=stream, tok16=True, fill_rows=R, dev_counts=cp, cu_cap=M, out_tokens=r["input_ids"].data_ptr(),
            attn_mask=r["attention_mask"].data_ptr(), position_ids=r["position_ids"].data_ptr(), pos_is_i64=True,
            segment_ids=r["segment_ids"].data_ptr(), cu_seqlens_out=r["cu_seqlens"].data_ptr())
    runs = []
    for rep in range(repeats):
        t = {"descriptor": rotating([c["descriptor"] for c in cases]),
             "pack_plan": rotating([c["plan_kernel"] for c in cases]),
             "device_counts_pack": rotating([c["device_pack"] for c in cases]),
             "host_plan_pack": rotating([lambda c=c: host_pack(c) for c in cases]),
             "device_route": rotating([lambda c=c: device_route(c) for c in cases])}
        runs.append(t)
        print(json.dumps({"kernel": "tokens_plan", "repeat": rep,
                          **{k + "_us": round(v * 1e6, 2) for k, v in t.items()}}), flush=True)
    med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
    T_mean = float(np.mean([c["T"] for c in cases]))
    print(json.dumps({
        "kernel": "tokens_plan summary", "sequences": B, "seq_len": S, "token_dtype": "uint16", "rows": R,
        "max_segs": M, "tokens": T_mean, "repeats": repeats,
        **{k + "_us_median": round(v * 1e6, 2) for k, v in med.items()},
        **{k + "_us_min_max": [round(min(t[k] for t in runs) * 1e6, 2), round(max(t[k] for t in runs) * 1e6, 2)]
           for k in med},
        "descriptor_plus_plan_us_median": round((med["descriptor"] + med["pack_plan"]) * 1e6, 2),
        "device_route_tokens_per_s": round(T_mean / med["device_route"], 1),
        "host_plan_pack_tokens_per_s": round(T_mean / med["host_plan_pack"], 1)}), flush=True)


def token_labels(dev, repeats=5) -> None:
    """Next-token labels at the ``tokens_indexed`` shape (uint16 corpus of 131072 sequences, 2048 per batch, seq_len
    4096): the indexed and the flat kernel, pad and pack mode, each with labels off, labels on (the fused store)
    and labels off followed by ``ops.ref_token_labels`` on the device tensors (what a caller writes without the
    option: a handful of torch kernels and their temporaries). 4 batches issued round-robin at launcher level, the
    flat stream gathered beforehand. The fused labels are compared with the composition first. One JSON line per
    repeat and a summary of medians."""
    from ddl_amd import _native
    from ddl_amd.ops.kernels import carve_token_outputs, segment_sources, token_output_bytes

    hip = _native.hip()
    rng = np.random.default_rng(0)
    n_src, B, S, rot = 131072, 2048, 4096, 4
    lens = rng.integers(256, 4097, size=n_src)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    corpus = torch.randint(0, 32768, (int(offs[-1]),), dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cases = []
    for _ in range(rot):
        idx = rng.choice(n_src, size=B, replace=False).astype(np.int64)
        start = np.ascontiguousarray(offs[idx])
        dofs = np.concatenate([[0], np.cumsum(offs[idx + 1] - offs[idx])]).astype(np.int64)
        rs, re_, so = ops.pack_plan(dofs, S)
        R, n_seg = len(rs), len(so) - 1
        seg_src = np.ascontiguousarray(segment_sources(start, dofs, so, n_seg))
        d = {k: torch.from_numpy(v).to(dev) for k, v in dict(start=start, dofs=dofs, rs=rs, re=re_, so=so,
                                                             seg_src=seg_src).items()}
        flat, _ = ops.gather_ragged(corpus, offs, idx)
        outs = {"pad": carve_token_outputs(torch.empty(token_output_bytes(B, S, None, labels=True), dtype=torch.uint8,
                                                       device=dev), B, S, None, labels=True),
                "pack": carve_token_outputs(torch.empty(token_output_bytes(R, S, n_seg, labels=True),
                                                        dtype=torch.uint8, device=dev), R, S, n_seg, labels=True)}
        cases.append((d, flat, outs, R, n_seg, int(dofs[-1])))

    def launch(c, kind, mode, labels):
        d, flat, outs, R, n_seg, _ = c
        ids, mask, pos, seg, cu, lab = outs[mode]
        pack = mode == "pack"
        kw = dict(offsets=0 if pack else d["dofs"].data_ptr(), row_start=d["rs"].data_ptr() if pack else 0,
                  row_end=d["re"].data_ptr() if pack else 0, seg_offsets=d["so"].data_ptr() if pack else 0,
                  n_seg=n_seg if pack else 0, out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(),
                  position_ids=pos.data_ptr(), pos_is_i64=True, segment_ids=seg.data_ptr() if pack else 0,
                  cu_seqlens_out=cu.data_ptr() if pack else 0, rows=R if pack else B, seq_len=S, pad_id=0,
                  mode=1 if pack else 0, stream=stream, tok16=True, labels=lab.data_ptr() if labels else 0)
        if kind == "indexed":
            hip.pad_pack_tokens_indexed(corpus=corpus.data_ptr(), corpus_elems=corpus.numel(),
                                        src_start=d["start"].data_ptr(), seg_src=d["seg_src"].data_ptr() if pack else 0,
                                        **kw)
        else:
            hip.pad_pack_tokens(tokens=flat.data_ptr(), **kw)

    def composed(c, kind, mode):
        launch(c, kind, mode, False)
        ids, mask, _, seg, _, _ = c[2][mode]
        return ops.ref_token_labels(ids, mask, seg)

    variants = [(kind, mode) for kind in ("indexed", "flat") for mode in ("pad", "pack")]
    for c in cases:  # the fused labels are the composition's
        for kind, mode in variants:
            launch(c, kind, mode, True)
            ref = composed(c, kind, mode)
            torch.cuda.synchronize()
            assert torch.equal(c[2][mode][5], ref), f"{kind} {mode}: fused labels differ from ref_token_labels"
    runs = []
    for r in range(repeats):
        t = {}
        for kind, mode in variants:
            t[f"{kind}_{mode}_off"] = rotating([lambda c=c: launch(c, kind, mode, False) for c in cases])
            t[f"{kind}_{mode}_on"] = rotating([lambda c=c: launch(c, kind, mode, True) for c in cases])
            t[f"{kind}_{mode}_off_plus_torch"] = rotating([lambda c=c: composed(c, kind, mode) for c in cases])
        runs.append(t)
        print(json.dumps({"kernel": "token labels", "repeat": r,
                          **{k + "_us": round(v * 1e6, 2) for k, v in t.items()}}), flush=True)
    med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
    R_mean = float(np.mean([c[3] for c in cases]))
    T_mean = float(np.mean([c[5] for c in cases]))
    print(json.dumps({
        "kernel": "token labels summary", "sequences": B, "seq_len": S, "token_dtype": "uint16", "pack_rows": R_mean,
        "tokens": T_mean, "repeats": repeats, **{k + "_us_median": round(v * 1e6, 2) for k, v in med.items()},
        **{f"{kind}_{mode}_on_over_off": round(med[f"{kind}_{mode}_on"] / med[f"{kind}_{mode}_off"], 3)
           for kind, mode in variants},
        **{f"{kind}_{mode}_on_over_torch": round(med[f"{kind}_{mode}_on"] / med[f"{kind}_{mode}_off_plus_torch"], 3)
           for kind, mode in variants}}), flush=True)


def token_stream(dev, repeats=5) -> None:
    """The token stream kernels. (1) ``token_stream_table`` (three launches, the Feistel order inline) at the
    ``bench_tokens.py`` corpus's document count and at 2^24 documents, against the torch composition of the same
    scan -- ``index_select`` of the lengths by a precomputed device index, then ``cumsum`` -- which needs that
    n-sized index built and uploaded per epoch (not timed here). (2) ``token_stream_plan`` at 64 and 2048 rows of
    4096 tokens over the ``tokens_plan`` corpus (131072 documents), against ``token_batch_descriptor`` +
    ``pack_plan_device`` at 64 and 2048 sequences, and the whole two-launch stream route (plan + pack). (3) The
    shuffled-row plan ``token_stream_plan_rows`` (two launches) and its three-launch route at the same sizes, in
    the same rounds as the contiguous plan and route, and the emit kernel alone over either plan. 4 windows issued
    round-robin at launcher level: device times."""
    from ddl_amd import _native
    from ddl_amd.ops.kernels import (_align16, _index_kw, _launch_stream_emit, _stream_plan_layout,
                                     device_plan_bytes, launch_stream_plan, launch_stream_plan_rows,
                                     stream_max_segments, token_stream_bytes)

    hip = _native.hip()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(0)
    for n in (8192, 1 << 24):
        lens = rng.integers(256, 4097, size=n)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        coffs = torch.from_numpy(offs).to(dev)
        perm = FeistelPermutation(n, 3, 1)
        idx = torch.from_numpy(perm(np.arange(n, dtype=np.int64))).to(dev)
        lens_dev = torch.from_numpy(lens.astype(np.int64)).to(dev)
        table = torch.empty(n + 1, dtype=torch.int64, device=dev)
        scratch = torch.empty(hip.token_stream_table_scratch(n), dtype=torch.int64, device=dev)
        sel = _index_kw(None, perm, 0)

        def kernel():
            hip.token_stream_table(corpus_offsets=coffs.data_ptr(), n_corpus=n, n=n, table=table.data_ptr(),
                                   tile_sums=scratch.data_ptr(), stream=stream, **sel)

        def composed():
            return torch.cumsum(lens_dev.index_select(0, idx), 0)

        kernel()
        assert torch.equal(table[1:], composed()), "table and torch composition differ"
        runs = [{"kernel": bench(kernel, reps=20), "torch": bench(composed, reps=20)} for _ in range(repeats)]
        med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
        print(json.dumps({"kernel": "token_stream_table", "documents": n, "repeats": repeats,
                          "kernel_us_median": round(med["kernel"] * 1e6, 2),
                          "kernel_us_min_max": [round(min(t["kernel"] for t in runs) * 1e6, 2),
                                                round(max(t["kernel"] for t in runs) * 1e6, 2)],
                          "torch_index_select_cumsum_us_median": round(med["torch"] * 1e6, 2),
                          "torch_us_min_max": [round(min(t["torch"] for t in runs) * 1e6, 2),
                                               round(max(t["torch"] for t in runs) * 1e6, 2)],
                          "kernel_over_torch": round(med["kernel"] / med["torch"], 3)}), flush=True)
        del coffs, idx, lens_dev, table, scratch

    n_src, S, rot = 131072, 4096, 4
    lens = rng.integers(256, 4097, size=n_src)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    corpus = torch.randint(0, 32768, (int(offs[-1]),), dtype=torch.int16, device=dev)
    coffs = torch.from_numpy(offs).to(dev)
    perm = FeistelPermutation(n_src, 3, 1)
    sel = _index_kw(None, perm, 0)
    table = ops.token_stream_table(coffs, perm)
    for B in (64, 2048):
        M = stream_max_segments(lens, B, S)
        plan_b, batch_b = token_stream_bytes(B, S, M)
        plans = [torch.empty(plan_b, dtype=torch.uint8, device=dev) for _ in range(rot)]
        wholes = [torch.empty(batch_b, dtype=torch.uint8, device=dev) for _ in range(rot)]

        def route(k):
            return launch_stream_plan(plans[k].data_ptr(), wholes[k], corpus_ptr=corpus.data_ptr(),
                                      corpus_elems=corpus.numel(), tok16=True, corpus_offsets_ptr=coffs.data_ptr(),
                                      n_corpus=n_src, table_ptr=table.data_ptr(), selector=sel, row_base=(3 + k) * B,
                                      rows=B, seq_len=S, pad_id=0, max_segs=M, stream=stream)

        def plan_only(k):
            p = plans[k].data_ptr()
            o_so = p + _align16(8 * M)
            o_rs = o_so + _align16(8 * (M + 1))
            hip.token_stream_plan(table=table.data_ptr(), corpus_offsets=coffs.data_ptr(), n_corpus=n_src, n=n_src,
                                  row_base=(3 + k) * B, rows=B, seq_len=S, max_segs=M, seg_offsets=o_so, seg_src=p,
                                  row_start=o_rs, row_end=o_rs + _align16(8 * B),
                                  counts=wholes[k][batch_b - 32:].data_ptr(), stream=stream, **sel)

        # the sequence-batched plan at the same step size: descriptor + in-order pack plan of B sequences
        dplans = [torch.empty(device_plan_bytes(B, B, B), dtype=torch.uint8, device=dev) for _ in range(rot)]
        dcounts = torch.empty(4 * rot, dtype=torch.int64, device=dev)

        def seq_plan(k):
            p = dplans[k].data_ptr()
            o_off = p + _align16(8 * B)
            o_ss = o_off + _align16(8 * (B + 1))
            o_so = o_ss + _align16(8 * B)
            o_rs = o_so + _align16(8 * (B + 1))
            o_re = o_rs + _align16(8 * B)
            cp = dcounts.data_ptr() + 32 * k
            hip.token_batch_descriptor(corpus_offsets=coffs.data_ptr(), n_corpus=n_src, n=B, seq_len=S, max_segs=B,
                                       src_start=p, offsets=o_off, seg_src=o_ss, counts=cp, pad_counts=False,
                                       stream=stream, **_index_kw(None, perm, (3 + k) * B))
            hip.pack_plan_device(offsets=o_off, n=B, seq_len=S, max_segs=B, max_rows=B, seg_offsets=o_so,
                                 row_start=o_rs, row_end=o_re, counts=cp, scratch=o_re + _align16(8 * B),
                                 stream=stream)

        r = route(0)
        torch.cuda.synchronize()
        assert r["counts"].tolist()[::2] == [B, B * S] and bool(r["attention_mask"].all()), "stream batch not dense"
        runs = [{"stream_plan": rotating([lambda k=k: plan_only(k) for k in range(rot)]),
                 "descriptor_plus_pack_plan": rotating([lambda k=k: seq_plan(k) for k in range(rot)]),
                 "stream_route": rotating([lambda k=k: route(k) for k in range(rot)])} for _ in range(repeats)]
        med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
        print(json.dumps({
            "kernel": "token_stream_plan", "rows": B, "seq_len": S, "documents": n_src, "max_segs": M,
            "segments": int(r["counts"][1]), "repeats": repeats,
            **{k + "_us_median": round(v * 1e6, 2) for k, v in med.items()},
            **{k + "_us_min_max": [round(min(t[k] for t in runs) * 1e6, 2), round(max(t[k] for t in runs) * 1e6, 2)]
               for k in med},
            "stream_route_tokens_per_s": round(B * S / med["stream_route"], 1)}), flush=True)

        # shuffled rows (token_stream_plan_rows: two launches, one wave per row) next to the contiguous plan, and
        # the emit kernel alone over a plan of scattered rows and over one of contiguous rows
        n_rows = int(offs[-1]) // S
        row_perm = FeistelPermutation(n_rows, 5, 1)
        Mr = stream_max_segments(lens, B, S, shuffled_rows=True)
        rplan_b, rbatch_b = token_stream_bytes(B, S, Mr, shuffled_rows=True)
        rplans = [torch.empty(rplan_b, dtype=torch.uint8, device=dev) for _ in range(rot)]
        rwholes = [torch.empty(rbatch_b, dtype=torch.uint8, device=dev) for _ in range(rot)]
        common = dict(corpus_ptr=corpus.data_ptr(), corpus_elems=corpus.numel(), tok16=True, rows=B, seq_len=S,
                      pad_id=0, stream=stream)
        plan_args = dict(corpus_offsets_ptr=coffs.data_ptr(), n_corpus=n_src, table_ptr=table.data_ptr(), selector=sel)

        def rows_route(k):
            return launch_stream_plan_rows(rplans[k].data_ptr(), rwholes[k], row_selector=_index_kw(None, row_perm,
                                                                                                    (3 + k) * B),
                                           stream_rows=n_rows, max_segs=Mr, **plan_args, **common)

        def rows_plan_only(k):
            o_ss, o_so, o_rs, o_re, o_scr = _stream_plan_layout(rplans[k].data_ptr(), B, Mr)
            rsel = {"rows_" + key: v for key, v in _index_kw(None, row_perm, (3 + k) * B).items()}
            hip.token_stream_plan_rows(table=table.data_ptr(), corpus_offsets=coffs.data_ptr(), n_corpus=n_src,
                                       n=n_src, stream_rows=n_rows, rows=B, seq_len=S, max_segs=Mr, seg_offsets=o_so,
                                       seg_src=o_ss, row_start=o_rs, row_end=o_re, scratch=o_scr,
                                       counts=rwholes[k][rbatch_b - 32:].data_ptr(), stream=stream, **sel, **rsel)

        def emit_only(k, shuffled):  # over the plan the route left in the window
            plan_ptr, whole, cap = ((rplans[k].data_ptr(), rwholes[k], Mr) if shuffled
                                    else (plans[k].data_ptr(), wholes[k], M))
            _launch_stream_emit(hip, whole, _stream_plan_layout(plan_ptr, B, cap), max_segs=cap,
                                position_dtype=torch.int64, labels=False, ignore_index=-100,
                                plan_fn=lambda **kw: None, plan_kw={}, **common)

        for k in range(rot):
            route(k)
            rr = rows_route(k)
        torch.cuda.synchronize()
        assert rr["counts"].tolist()[::2] == [B, B * S] and bool(rr["attention_mask"].all()), "row batch not dense"
        runs = [{"rows_plan": rotating([lambda k=k: rows_plan_only(k) for k in range(rot)]),
                 "stream_plan": rotating([lambda k=k: plan_only(k) for k in range(rot)]),
                 "rows_route": rotating([lambda k=k: rows_route(k) for k in range(rot)]),
                 "stream_route": rotating([lambda k=k: route(k) for k in range(rot)]),
                 "emit_scattered_rows": rotating([lambda k=k: emit_only(k, True) for k in range(rot)]),
                 "emit_contiguous_rows": rotating([lambda k=k: emit_only(k, False) for k in range(rot)])}
                for _ in range(repeats)]
        med = {k: float(np.median([t[k] for t in runs])) for k in runs[0]}
        print(json.dumps({
            "kernel": "token_stream_plan_rows", "rows": B, "seq_len": S, "documents": n_src, "max_segs": Mr,
            "segments": int(rr["counts"][1]), "repeats": repeats,
            **{k + "_us_median": round(v * 1e6, 2) for k, v in med.items()},
            **{k + "_us_min_max": [round(min(t[k] for t in runs) * 1e6, 2), round(max(t[k] for t in runs) * 1e6, 2)]
               for k in med},
            "rows_route_tokens_per_s": round(B * S / med["rows_route"], 1)}), flush=True)


if __name__ == "__main__":
    if "--only-token-stream" in sys.argv[1:]:  # profiles/token_stream/
        token_stream(torch.device("cuda", 0))
        sys.exit(0)
    if "--only-token-labels" in sys.argv[1:]:  # profiles/token_labels/
        token_labels(torch.device("cuda", 0))
        sys.exit(0)
    if "--only-tokens-indexed" in sys.argv[1:]:  # the one case, e.g. for profiles/resident_tokens/
        tokens_indexed(torch.device("cuda", 0))
        sys.exit(0)
    if "--only-tokens-plan" in sys.argv[1:]:  # profiles/resident_tokens_plan/
        tokens_plan(torch.device("cuda", 0))
        sys.exit(0)
    sys.exit(main())
