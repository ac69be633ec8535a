"""Pad mode of the flat and the indexed pad/pack kernel at launcher level, at the ``tokens_indexed`` shape of
``benchmarks/kernels_bench.py`` (2048 sequences of a 570 MB uint16 corpus, seq_len 4096). It passes only the
keywords the bindings have always had, so it runs unchanged on an older tree: the before / after of a change to
the kernels (``profiles/token_labels``). One JSON line: medians of 5 x 48 rotating launches."""
import json

import numpy as np
import torch

from ddl_amd import _native, ops
from ddl_amd.ops.kernels import carve_token_outputs, token_output_bytes


def bench(fn, reps=48):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3


dev = torch.device("cuda", 0)
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
    start = torch.from_numpy(np.ascontiguousarray(offs[idx])).to(dev)
    flat, dofs = ops.gather_ragged(corpus, offs, idx)
    dofs = dofs.clone()
    out = carve_token_outputs(torch.empty(token_output_bytes(B, S, None), dtype=torch.uint8, device=dev), B, S, None)
    cases.append((start, flat, dofs, out))


def launch(c, indexed):
    start, flat, dofs, (ids, mask, pos, _, _) = c
    kw = dict(offsets=dofs.data_ptr(), row_start=0, row_end=0, seg_offsets=0, n_seg=0, out_tokens=ids.data_ptr(),
              attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(), pos_is_i64=True, segment_ids=0, cu_seqlens_out=0,
              rows=B, seq_len=S, pad_id=0, mode=0, stream=stream, tok16=True)
    if indexed:
        hip.pad_pack_tokens_indexed(corpus=corpus.data_ptr(), corpus_elems=corpus.numel(), src_start=start.data_ptr(),
                                    seg_src=0, **kw)
    else:
        hip.pad_pack_tokens(tokens=flat.data_ptr(), **kw)


res = {}
for name, indexed in (("indexed_pad_us", True), ("flat_pad_us", False)):
    i = [0]

    def one():
        launch(cases[i[0] % rot], indexed)
        i[0] += 1

    res[name] = round(float(np.median([bench(one) for _ in range(5)])), 2)
print(json.dumps({"kernel": "pad mode, labels off", **res}), flush=True)
