"""CPU: the capped ball query's selection rule (include/se3conv_capped.h) -- host-side argument checks, the message of a
library built before the entry points existed, the contract's check vectors and uniformity of the rule (two z-tests);
tests/test_abi_tables.py holds the header against its table, the library and its hostile-memory module."""
import ctypes as C

import numpy as np
import pytest

from capped_neighbours import edge_hash, edge_key, mix32


def test_a_library_without_the_capped_symbols_asks_for_a_rebuild(built_library, monkeypatch):
    from se3conv3d_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.CAPPED_SIGNATURES, "se3_ball_query_capped_that_is_not_there", (C.c_int, []))
    with pytest.raises(_lib.Se3LibraryError, match="rebuild"):
        _lib.load()


def test_host_side_argument_checks(built_library):
    from se3conv3d_amd import _lib

    lib = _lib.load()
    null, some = C.c_void_p(0), C.c_void_p(256)

    def call(capacity=10, info=some, m=8, radius=0.1, ws=null, ws_bytes=0, n=10):
        return lib.se3_ball_query_capped(null, null, null, null, null, null, radius, n, n, 1, null, 0, 0, ws, ws_bytes, capacity,
                                         null, null, null, info, null, m, 0, null, null)

    assert call() == -1                      # null points, offsets and workspace
    assert call(info=null) == -1
    assert call(capacity=-1) == -1
    assert call(radius=0.0) == -1
    assert call(n=-1) == -1
    assert call(m=65) == -2                  # the stated limit: SE3_ERR_UNSUPPORTED
    assert call(ws=some, ws_bytes=64) == -3  # a workspace that is too small is refused before anything is launched
    q = lib.se3_ball_query_capped_workspace_bytes
    assert q(1000, 1000) >= lib.se3_ball_query_workspace_bytes(1000, 1000) + 1000 * 8 and q(0, 0) > 0


def test_check_vectors():
    for (seed, s, p), want in (((0, 0, 0), 0x0), ((1, 2, 3), 0x69157D8E), ((12345, 65535, 99999), 0x044B2766),
                               ((0xFFFFFFFF, 1499, 5999), 0x72C91147)):
        assert int(edge_hash(seed, s, p)) == want
        assert int(edge_key(seed, s, p)) == (want << 32) | p
    assert int(mix32(0)) == 0 and int(mix32(1)) == 0x514E28B7     # murmur3 fmix32(1)
    # vectorised = scalar
    s, p = np.arange(7), np.arange(7) * 11
    assert [int(v) for v in edge_hash(9, s, p)] == [int(edge_hash(9, int(a), int(b))) for a, b in zip(s, p)]


# c = 40 candidates, m = 8 kept, S = 20 000 consecutive samples over one candidate set.  A uniform rule exceeds |z| = 5
# with probability < 1e-4 over all ranks and seeds (2 * (1 - Phi(5)) * 40 ranks * 4 seeds * 2 candidate sets = 1.8e-4 / 2).
C_HITS, M_KEPT, SAMPLES = 40, 8, 20000
CANDIDATE_SETS = {"consecutive ids": np.arange(C_HITS, dtype=np.int64),
                  "scattered ids": np.sort(np.random.RandomState(7).choice(100000, C_HITS, replace=False)).astype(np.int64)}


def kept_matrix(seed, cand, first_sample=0):
    s = np.arange(first_sample, first_sample + SAMPLES, dtype=np.int64)[:, None]
    keys = edge_key(seed, np.broadcast_to(s, (SAMPLES, C_HITS)), np.broadcast_to(cand[None, :], (SAMPLES, C_HITS)))
    tau = np.partition(keys, M_KEPT - 1, axis=1)[:, M_KEPT - 1:M_KEPT]
    kept = keys <= tau
    assert (kept.sum(1) == M_KEPT).all()
    return kept


@pytest.mark.parametrize("which", sorted(CANDIDATE_SETS))
@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 32 - 1])
def test_every_rank_is_selected_as_often_as_a_uniform_draw_selects_it(seed, which):
    kept = kept_matrix(seed, CANDIDATE_SETS[which])
    q = M_KEPT / C_HITS
    z = (kept.sum(0) - SAMPLES * q) / np.sqrt(SAMPLES * q * (1 - q))      # Binomial(S, m / c) per rank
    print(f"seed {seed}, {which}: max |z| over the ranks = {np.abs(z).max():.2f}")
    assert np.abs(z).max() <= 5.0


@pytest.mark.parametrize("which", sorted(CANDIDATE_SETS))
@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 32 - 1])
def test_consecutive_samples_draw_independent_subsets(seed, which):
    kept = kept_matrix(seed, CANDIDATE_SETS[which])
    overlap = (kept[1:] & kept[:-1]).sum(1)
    m, c = M_KEPT, C_HITS
    mean = m * m / c                                                          # hypergeometric(c, m, m)
    var = m * (m / c) * (1 - m / c) * (c - m) / (c - 1)
    z = (overlap.mean() - mean) / np.sqrt(var / overlap.size)
    print(f"seed {seed}, {which}: mean overlap {overlap.mean():.4f} against {mean:.4f}, z = {z:.2f}")
    assert abs(z) <= 5.0

