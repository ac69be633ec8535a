"""Independent references and case tables for the reduction and owner-bucketing kernels
(csrc/kernels/misc.hip, csrc/kernels/bucket.hip).

Nothing here calls a project op: the references are numpy on the CPU, in float64 or exact integers, written
from the ops' documented meaning. ``tests/test_reductions.py`` runs the tables through the CPU paths and the
host twins, ``tests/test_reductions_gpu.py`` and ``tests/test_bucketing_gpu.py`` through the HIP kernels. The
checksum's oracle is ``ops.ref_checksum`` (a numpy sum of the 32-bit words).
"""

from __future__ import annotations

import functools

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)


# --------------------------------------------------------------- column_stats
def ulp32(v) -> np.ndarray:
    """The float32 spacing at |v| (float64 array): what one unit in the last place of a float32 result near
    ``v`` is worth."""
    a = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def ref_column_stats(x) -> dict:
    """Float64 statistics of the float32 table ``x`` [n, c]: ``mean`` and population ``std`` (two-pass, about
    the float64 mean), exact float32 ``min`` / ``max``, and the float32 spacings the bounds use:
    ``ulp_mean = ulp32(mean)`` and ``ulp_floor = ulp32(|mean| + |std|)``."""
    a = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert a.dtype == np.float32 and a.ndim == 2
    d = a.astype(np.float64)
    mean = d.mean(0)
    std = np.sqrt(((d - mean) ** 2).mean(0))
    return {"mean": mean, "std": std, "min": a.min(0), "max": a.max(0), "ulp_mean": ulp32(mean),
            "ulp_floor": ulp32(np.abs(mean) + np.abs(std))}


# (offset, sd) of the random columns; the first four are the pairs measured on the CPU path
RANDOM_KINDS = ((3.0, 1.0), (1000.0, 1.0), (100.0, 0.1), (1e4, 1.0),
                (0.0, 1.0), (-3.0, 2.0), (-1000.0, 1.0), (1e-3, 1e-5))
FIXED_KINDS = ("const 1000", "const -2.5", "all negative", "all positive", "one value then zeros", "flt_max/4")
KINDS = RANDOM_KINDS + FIXED_KINDS
MINMAX_ONLY = "flt_max/4"  # mean and std of this column are not asserted

# rows x cols, one per dispatch path of the kernels (narrow: cols <= 256, 256 threads per block, grid capped at
# 256 blocks, 4-way unrolled loop + tail loop; wide: 64-column tiles x row blocks of <= 4096 rows, 4 waves)
STATS_SHAPES = (
    (1, 9), (3, 9),        # fewer elements than one stride: tail loop only
    (7777, 9),             # active = 252: both loops
    (120_000, 9),          # grid capped at 256 blocks
    (4096, 1),             # one column
    (3000, 128),           # cols divides 256
    (3000, 200), (3000, 255), (2000, 256),  # one thread per column per block
    (3, 257), (999, 300),  # wide: fewer rows than waves; a partial last tile
    (4100, 320),           # wide: two row blocks, full tiles
    (4097, 257),           # wide: two row blocks, a one-column last tile
)


def column_kind(j: int, start: int = 0):
    return KINDS[(j + start) % len(KINDS)]


def kind_starts(cols: int) -> tuple:
    """Rotations of the kind table that together put every kind into a table of ``cols`` columns."""
    return tuple(range(0, len(KINDS), cols)) if cols < len(KINDS) else (0,)


@functools.lru_cache(maxsize=None)
def stats_table(rows: int, cols: int, start: int = 0) -> np.ndarray:
    """The float32 [rows, cols] test table (read-only): column j is of kind ``column_kind(j, start)``, generated
    in float64 from a fixed seed and stored as float32."""
    rng = np.random.default_rng(1000 * rows + 7 * cols + start)
    t = np.empty((rows, cols), dtype=np.float64)
    for j in range(cols):
        k = column_kind(j, start)
        z = rng.standard_normal(rows)
        if isinstance(k, tuple):
            t[:, j] = k[0] + k[1] * z
        elif k == "const 1000":
            t[:, j] = 1000.0
        elif k == "const -2.5":
            t[:, j] = -2.5
        elif k == "all negative":
            t[:, j] = -(np.abs(z) * 7 + 0.5)
        elif k == "all positive":
            t[:, j] = np.abs(z) * 7 + 0.5
        elif k == "one value then zeros":
            t[:, j] = 0.0
            t[0, j] = 1000.0
        else:  # +FLT_MAX/4 at one row, -FLT_MAX/4 at another (where there is one)
            t[:, j] = z
            t[rows // 3, j] = FLT_MAX / 4
            if rows > 1:
                t[rows // 3 + (rows + 1) // 3, j] = -FLT_MAX / 4
    out = t.astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stats_ref(rows: int, cols: int, start: int = 0) -> dict:
    return ref_column_stats(stats_table(rows, cols, start))


def offset_table(offset: float, sd: float, rows: int = 20_000, cols: int = 9) -> np.ndarray:
    """``offset + sd * randn`` in every column (float64, then float32), fixed seed."""
    rng = np.random.default_rng(5)
    return (offset + sd * rng.standard_normal((rows, cols))).astype(np.float32)


def check_column_stats(stats: dict, ref: dict, kinds, report=None) -> None:
    """The bounds of the reduction suites on ``ops.column_stats`` output ``stats`` against ``ref_column_stats``
    output ``ref``; ``kinds[j]`` names column j. ``report``: a dict that collects the worst errors per kind.

    * min and max equal the reference bit for bit;
    * ``|mean - mean_ref| <= 1e-4 * std_ref + ulp32(mean_ref)``: the absolute tolerance the suite always had on
      unit-scale data, scaled by the column's spread, plus one unit of the float32 result;
    * ``|std - std_ref| <= 1e-3 * std_ref + 4 * ulp32(|mean_ref| + |std_ref|)``: the suite's relative tolerance,
      and a floor because spread below a few float32 spacings of the column's magnitude is not in the input.
    """
    mn, mx = stats["min"].cpu(), stats["max"].cpu()
    assert mn.dtype == mx.dtype == torch.float32
    assert torch.equal(mn, torch.from_numpy(ref["min"])), "min differs from the exact minimum"
    assert torch.equal(mx, torch.from_numpy(ref["max"])), "max differs from the exact maximum"
    mean = stats["mean"].cpu().double().numpy()
    std = stats["std"].cpu().double().numpy()
    e_mean, e_std = np.abs(mean - ref["mean"]), np.abs(std - ref["std"])
    b_mean = 1e-4 * ref["std"] + ref["ulp_mean"]
    b_std = 1e-3 * ref["std"] + 4 * ref["ulp_floor"]
    bad = []
    for j, k in enumerate(kinds):
        if k == MINMAX_ONLY:
            continue
        if report is not None:
            w = report.setdefault(k, [0.0, 0.0])  # worst error / bound
            w[0], w[1] = max(w[0], e_mean[j] / b_mean[j]), max(w[1], e_std[j] / b_std[j])
        if not e_mean[j] <= b_mean[j]:
            bad.append(f"col {j} ({k}): mean {mean[j]!r} vs {ref['mean'][j]!r}, error {e_mean[j]:.3g} > {b_mean[j]:.3g}")
        if not e_std[j] <= b_std[j]:
            bad.append(f"col {j} ({k}): std {std[j]!r} vs {ref['std'][j]!r}, error {e_std[j]:.3g} > {b_std[j]:.3g} "
                       f"(relative {e_std[j] / max(ref['std'][j], 1e-300):.3g})")
    assert not bad, "\n".join(bad[:8])


# ------------------------------------------------------------ owner bucketing
# n, gb, world: the suite's first four cases, then lb > 1024 (the cross-chunk carry of bucket_recv), a partial
# chunk, world 1, and worlds whose last ranks own few or no rows
BUCKET_CASES = (
    (777, 48, 4), (100_000, 2048, 8), (5000, 512, 2), (64, 64, 64),
    (20_000, 4096, 2),   # lb = 2048: two full chunks in bucket_recv
    (20_000, 5000, 2),   # lb = 2500: a partial third chunk; gb no multiple of 1024 in bucket_send
    (9_000, 8192, 4),    # lb = 2048 with four sources carrying over chunks
    (1025, 1025, 1),     # world 1; one position past a chunk
    (130, 128, 64),      # lb = 2; shard 3: the last ranks own few or no rows
    (70, 64, 64),        # shard 2: ranks 35..63 own nothing (empty send lists, zero counts)
)
BUCKET_SEED = 9


def bucket_geometry(n: int, gb: int, world: int) -> tuple:
    """(lb, shard, number of global batches the suites run): position i of a batch goes to rank i // lb, sample
    idx lives on rank idx // shard."""
    return gb // world, -(-n // world), min(2, n // gb)


def ref_owner_maps(perm, n: int, g: int, gb: int, world: int, rank: int) -> tuple:
    """(send_rows, inv, send_counts, recv_counts) of rank ``rank`` for global batch ``g`` of ``perm``, from
    numpy alone.

    ``owner = idx // shard``. ``send_rows``: the rank's own samples among the batch's ``gb`` positions, in
    position order, as shard-local rows. ``inv[j]``: where position j of the rank's slice sits in the all-to-all
    receive buffer, which is grouped by source rank and in position order within a source (a stable argsort of
    the slice's owners). ``send_counts[d]``: rows sent to rank d; ``recv_counts[q]``: rows received from q."""
    lb, shard = gb // world, -(-n // world)
    idx = perm.numpy_eval(np.arange(g * gb, (g + 1) * gb, dtype=np.int64))
    owner = idx // shard
    mine = owner == rank
    send_rows = idx[mine] - rank * shard
    dest = np.arange(gb) // lb
    send_counts = np.bincount(dest[mine], minlength=world)[:world].astype(np.int64)
    sl = owner[rank * lb:(rank + 1) * lb]
    inv = np.empty(lb, dtype=np.int64)
    inv[np.argsort(sl, kind="stable")] = np.arange(lb)
    recv_counts = np.bincount(sl, minlength=world).astype(np.int64)
    return send_rows, inv, send_counts, recv_counts
