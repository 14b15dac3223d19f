"""CPU restatement of the capped ball query's selection rule (include/se3conv_capped.h), written from the contract's text
and not from the kernel (a helper module like seeded_params.py, not a conftest).

  mix(x): murmur3's 32-bit finaliser;  h = mix(mix(seed ^ mix(s)) + p * 0x9E3779B9);  key(s, p) = (h << 32) | p
  a sample with more than m hits keeps the m with the smallest keys, in the order the uncapped list has them."""
from __future__ import annotations

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """murmur3 finaliser on (arrays of) 32-bit words, computed in uint64 and masked."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def edge_hash(seed, s, p):
    """h of the contract; ``seed`` is the effective seed (host seed + device word, mod 2^32)."""
    seed = np.uint64(int(seed) & 0xFFFFFFFF)
    s = np.asarray(s, dtype=np.int64).astype(np.uint64) & M32
    p = np.asarray(p, dtype=np.int64).astype(np.uint64) & M32
    return mix32((mix32(seed ^ mix32(s)) + p * np.uint64(0x9E3779B9)) & M32)


def edge_key(seed, s, p):
    p64 = np.asarray(p, dtype=np.int64).astype(np.uint64) & M32
    return (edge_hash(seed, s, p) << np.uint64(32)) | p64


def select_capped(neighbors: torch.Tensor, ends: torch.Tensor, m: int, seed: int):
    """The capped list of an UNCAPPED one (``neighbors [E,2]`` grouped by sample, inclusive ``ends [M]``):
    ``(neighbors, ends, degrees)`` with every sample's survivors in their original order."""
    nb = neighbors.detach().cpu().numpy().astype(np.int64)
    e = ends.detach().cpu().numpy().astype(np.int64)
    degrees = np.diff(e, prepend=0)
    if m <= 0:
        return neighbors.detach().cpu().clone(), ends.detach().cpu().clone(), torch.from_numpy(degrees.astype(np.int32))
    keys = edge_key(seed, nb[:, 0], nb[:, 1])
    keep = np.ones(nb.shape[0], dtype=bool)
    start = 0
    for s, end in enumerate(e):
        if end - start > m:
            k = keys[start:end]
            tau = np.partition(k, m - 1)[m - 1]
            keep[start:end] = k <= tau
        start = end
    out = nb[keep]
    new_ends = np.cumsum(np.minimum(degrees, m))
    return (torch.from_numpy(out).to(neighbors.dtype), torch.from_numpy(new_ends.astype(np.int32)),
            torch.from_numpy(degrees.astype(np.int32)))
