"""GPU: every search route and entry point of the ball query against the predicate (`O.ball_query`) on clouds that hold
pairs just inside the radius whose points the reference's cells (size = radius) put two apart (tests/boundary_pairs.py).
The predicate defines the edge set; a route that looks one reference cell to each side drops those pairs, which no
`torch.rand` cloud shows.  Edge sets and offsets are compared exactly."""
import functools

import pytest
import torch

import boundary_pairs as B
from capped_neighbours import select_capped
from conftest import canon_edges
from oracle import se3conv_oracle as O
from padded_cases import assert_padded_edges, word

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 0.07
FAR = {"cell_range": (1022, 1031), "axes": (0,)}      # pairs at the cells around the 32-bit keys' stride of 1024


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    amd.set_precision("bf16x3")
    return amd


class Case:
    """Clouds on the CPU, the planted edges as (sample, source) rows, and the oracle's list: built once per module."""

    def __init__(self, ps, bs, pd, bd, r, batches, planted):
        self.ps, self.bs, self.pd, self.bd, self.r, self.batches, self.planted = ps, bs, pd, bd, r, batches, planted
        self.self_cloud = pd is ps
        self.ref_nb, self.ref_ends = O.ball_query(ps, pd, bs, bd, r)
        self.e = int(self.ref_nb.shape[0])
        assert bool(B.has_edges(self.ref_nb, planted, ps.shape[0]).all()) and planted.shape[0] > 0

    def args(self):
        ps, bs = self.ps.to(DEV), self.bs.to(DEV)
        pd, bd = (ps, bs) if self.self_cloud else (self.pd.to(DEV), self.bd.to(DEV))
        return ps, pd, bs, bd, self.r


def _self_case(r, per_axis, sizes, extent, seed, **kw):
    """A cloud against itself with `sizes[b]` points in batch element b."""
    axes = len(kw.get("axes", (0, 1, 2)))
    fills = [n - 2 - 2 * axes * per_axis for n in sizes]
    ps, bs, pairs = B.boundary_pair_cloud(r, per_axis, fills, len(sizes), extent, seed, **kw)
    assert ps.shape[0] == sum(sizes)
    return ps, bs, pairs


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("all_pairs_2048", "grid_2049"):
        # the largest source set of the all-pairs route, and the same 2048 points plus one far point on the grid route
        ps, bs, pairs = _self_case(R, 64, [2048], 1.0, 1)
        if name == "grid_2049":
            ps, bs = torch.cat((ps, torch.tensor([[5.0, 5.0, 5.0]]))), torch.cat((bs, bs[-1:]))
        return Case(ps, bs, ps, bs, R, 1, B.both_directions(pairs))
    if name == "grid_32bit_1_batch":
        ps, bs, pairs = _self_case(R, 64, [2100], 40.0, 2)
        return Case(ps, bs, ps, bs, R, 1, B.both_directions(pairs))
    if name == "grid_32bit_2_batches":
        ps, bs, pairs = _self_case(R, 64, [1200, 1000], 1.0, 3)
        return Case(ps, bs, ps, bs, R, 2, B.both_directions(pairs))
    if name == "grid_64bit_3_batches":
        # the third batch element holds exactly the anchor and one pair (batch element 0's first, same anchor: same cells)
        ps, bs, pairs = _self_case(R, 64, [1500, 1097], 1.0, 4)
        n = ps.shape[0]
        ps = torch.cat((ps, ps[:1], ps[pairs[0]]))
        bs = torch.cat((bs, torch.full((3,), 2, dtype=torch.int32)))
        pairs = torch.cat((pairs, torch.tensor([[n + 1, n + 2]])))
        assert ps.shape[0] == 2600
        return Case(ps, bs, ps, bs, R, 3, B.both_directions(pairs))
    if name == "r001":
        ps, bs, pairs = _self_case(0.01, 64, [2100], 1.0, 5)
        return Case(ps, bs, ps, bs, 0.01, 1, B.both_directions(pairs))
    if name == "far_cells_r001":
        # r = 0.01 has such pairs beyond cell 1000 only over boxes that do not start at 0; there the sample is in cell 1024
        ps, bs, pairs = _self_case(0.01, 64, [2100], (12.0, 1.0, 1.0), 6, origin=(2.1532969, 0.0, 0.0), **FAR)
        return Case(ps, bs, ps, bs, 0.01, 1, B.both_directions(pairs))
    if name == "far_cells_r007":
        # samples in cells 1023 (its partner in 1021: below the clamp), 1025, 1027 and 1029 (clamped with their partners)
        ps, bs, pairs = _self_case(R, 64, [2100], (75.0, 1.0, 1.0), 7, origin=(3.2027559, 0.0, 0.0), **FAR)
        return Case(ps, bs, ps, bs, R, 1, B.both_directions(pairs))
    if name in ("down_up_32bit", "down_up_64bit"):
        return _two_cloud_case(2 if name == "down_up_32bit" else 3)
    raise KeyError(name)


def _two_cloud_case(batches):
    """A query between two clouds: the planted samples are samples only, their partners sources only.  Sources sit ON the
    low and the high faces of their box, with samples across those faces just inside the radius; further samples lie up to
    one radius outside the box on every side (their cells clamp)."""
    g = torch.Generator().manual_seed(20 + batches)
    pts, bid, pairs = B.boundary_pair_cloud(R, 64, 900 if batches == 2 else 600, batches, 1.0, 8 + batches)
    is_sample = torch.zeros(pts.shape[0], dtype=torch.bool)
    is_sample[pairs[:, 0]] = True
    top = float(pts[1, 0])                                      # the far corner: the sources' maximum on every axis
    src, src_b, dst, dst_b, planted = [], [], [], [], []
    for b in range(batches):
        mine = bid == b
        on_low, on_high = torch.rand(24, 3, generator=g), torch.rand(24, 3, generator=g)
        for axis in range(3):
            on_low[axis * 8:(axis + 1) * 8, axis] = 0.0
            on_high[axis * 8:(axis + 1) * 8, axis] = top
        across = torch.cat([B.farthest_hit(face[axis * 8:(axis + 1) * 8], axis, d, R)
                            for face, d in ((on_low, -1), (on_high, 1)) for axis in range(3)])
        around = torch.rand(300, 3, generator=g) * (top + 2 * R) - R
        # sources: anchor, corner, the partners, fill, the face points; samples: the planted samples, across, around
        k = int(is_sample[mine].sum())
        ids = torch.arange(k)
        planted.append(torch.stack((sum(t.shape[0] for t in dst) + ids, sum(t.shape[0] for t in src) + 2 + ids), dim=1))
        src.append(torch.cat((pts[mine & ~is_sample], on_low, on_high)))
        dst.append(torch.cat((pts[mine & is_sample], across, around)))
        src_b.append(torch.full((src[-1].shape[0],), b, dtype=torch.int32))
        dst_b.append(torch.full((dst[-1].shape[0],), b, dtype=torch.int32))
    ps, bs, pd, bd, planted = torch.cat(src), torch.cat(src_b), torch.cat(dst), torch.cat(dst_b), torch.cat(planted)
    assert ps.shape[0] > 2048
    assert torch.equal(pd[planted[:, 0]], pts[pairs[:, 0]]) and torch.equal(ps[planted[:, 1]], pts[pairs[:, 1]])
    c = Case(ps, bs, pd, bd, R, batches, planted)
    # the samples across the faces are neighbours of the face sources they were made from, and lie outside the box
    outside, faces = torch.cat([t[-348:-300] for t in dst]), torch.cat([t[-48:] for t in src])
    assert bool(B.predicate(outside, faces, R).all()) and bool(((outside < 0) | (outside > top)).any(1).all())
    return c


GRID_CASES = ["grid_2049", "grid_32bit_1_batch", "grid_32bit_2_batches", "grid_64bit_3_batches", "r001", "far_cells_r001",
              "far_cells_r007", "down_up_32bit", "down_up_64bit"]
ALL_CASES = ["all_pairs_2048"] + GRID_CASES


def assert_is_the_oracle_list(c, nb, ends):
    assert torch.equal(ends.cpu(), c.ref_ends)
    assert torch.equal(canon_edges(nb[:c.e]), canon_edges(c.ref_nb))
    assert bool(B.has_edges(nb[:c.e], c.planted, c.ps.shape[0]).all())     # (implied; names what a failure is about)


@pytest.mark.parametrize("name", ALL_CASES)
def test_two_phase_query_lists_the_predicate_set(amd, name):
    """se3_ball_query_count / _store: 64-bit keys on the grid route, whatever the number of batch elements."""
    c = case(name)
    assert amd.ops.ball_query_needs_grid(c.ps.shape[0]) == (name != "all_pairs_2048")
    nb, ends = amd.ops.ball_query(*c.args(), c.batches)
    assert nb.shape[0] == c.e
    assert_is_the_oracle_list(c, nb, ends)


@pytest.mark.parametrize("name", ALL_CASES)
def test_bounded_query_lists_the_predicate_set_and_truncates_as_documented(amd, name):
    """se3_ball_query_bounded: 32-bit keys with one or two batch elements, 64-bit keys with three."""
    c = case(name)
    nb, ends, info = amd.ops.ball_query_bounded(*c.args(), capacity=c.e + 7, n_batches=c.batches)
    assert info.tolist() == [c.e, 0]
    assert_is_the_oracle_list(c, nb, ends)
    # a capacity one below the edge count: the flag, the true count, clamped offsets, the head of the list
    cut, cut_ends, cut_info = amd.ops.ball_query_bounded(*c.args(), capacity=c.e - 1, n_batches=c.batches)
    assert cut_info.tolist() == [c.e, 1]
    assert torch.equal(cut_ends.cpu(), torch.clamp(c.ref_ends, max=c.e - 1)) and torch.equal(cut, nb[:c.e - 1])


def test_the_2048_points_have_the_same_edges_on_both_routes(amd):
    """2048 sources are searched all-pairs, 2049 through the grid: the edges among the shared 2048 points are the same."""
    small, large = case("all_pairs_2048"), case("grid_2049")
    assert torch.equal(small.ps, large.ps[:2048]) and not amd.ops.ball_query_needs_grid(2048) and amd.ops.ball_query_needs_grid(2049)
    lists = []
    for c in (small, large):
        nb, ends, info = amd.ops.ball_query_bounded(*c.args(), capacity=c.e, n_batches=1)
        nb = nb.cpu()
        assert info.tolist() == [c.e, 0] and bool(B.has_edges(nb, c.planted, c.ps.shape[0]).all())
        lists.append(canon_edges(nb[(nb[:, 0] < 2048) & (nb[:, 1] < 2048)]))
    assert torch.equal(lists[0], lists[1])
    assert lists[1].shape[0] == large.e - 1                    # (the far point has its self edge and no other)


@pytest.mark.parametrize("name", ["grid_32bit_2_batches", "grid_64bit_3_batches", "down_up_32bit", "down_up_64bit"])
def test_shared_source_grid_built_then_reused(amd, name):
    """se3_ball_query_bounded_shared with grid_valid = 0 (the call builds the grid) and then 1 (it searches the kept one)."""
    c = case(name)
    args = c.args()
    box = amd.ops.batch_aabb(args[0], args[2], c.batches)
    holder = amd.ops.SourceGrids()
    buffers = []
    for _ in range(2):
        nb, ends, info = amd.ops.ball_query_bounded(*args, capacity=c.e + 3, n_batches=c.batches, src_box=box, grids=holder)
        assert info.tolist() == [c.e, 0]
        assert_is_the_oracle_list(c, nb, ends)
        assert list(holder.grids) == [c.r]
        buffers.append(holder.grids[c.r][1])
    assert buffers[0] is buffers[1]                            # the second call was handed the first one's grid as valid


@pytest.mark.parametrize("name", ["all_pairs_2048", "grid_32bit_1_batch", "far_cells_r007"])
def test_padded_query_lists_no_pair_of_the_absent_rows(amd, name):
    """se3_ball_query_padded with the last planted pairs behind the row count: the present rows' list is the oracle's on
    the present rows, with their planted pairs; the absent rows -- real points, real pairs -- are not listed."""
    c = case(name)
    n = c.ps.shape[0]
    pairs = c.planted[:c.planted.shape[0] // 2]                # (sample, partner), one direction
    absent = pairs[-24:].reshape(-1)
    keep = torch.ones(n, dtype=torch.bool)
    keep[absent] = False
    order = torch.cat((torch.nonzero(keep)[:, 0], absent))     # the same cloud with those 48 points last
    valid = n - absent.numel()
    ps, bs = c.ps[order].contiguous(), c.bs[order].contiguous()
    new_id = torch.empty(n, dtype=torch.int64)
    new_id[order] = torch.arange(n)
    present = new_id[B.both_directions(pairs[:-24])]
    ref_nb, ref_ends = O.ball_query(ps[:valid], ps[:valid], bs[:valid], bs[:valid], c.r)
    assert bool(B.has_edges(ref_nb, present, n).all())
    p, b, w = ps.to(DEV), bs.to(DEV), word(valid)
    nb, ends, info = amd.ops.ball_query_padded(p, p, b, b, c.r, ref_nb.shape[0] + 5, 1, n_valid_src=w, n_valid_dst=w)
    assert_padded_edges(nb, ends, info, ref_nb, ref_ends, valid, valid)
    assert bool(B.has_edges(nb[:ref_nb.shape[0]], present, n).all())


@pytest.mark.parametrize("name", ["all_pairs_2048", "grid_32bit_2_batches", "grid_64bit_3_batches", "down_up_32bit"])
def test_capped_query_counts_and_keeps_oracle_edges(amd, name):
    c = case(name)
    n_dst = c.pd.shape[0]
    counts = torch.diff(c.ref_ends, prepend=torch.zeros(1, dtype=torch.int32))
    assert 4 < int(counts.max()) <= 64
    # a cap above every degree: the same set
    nb, ends, info, deg = amd.ops.ball_query_capped(*c.args(), 64, 1234, capacity=n_dst * 64, n_batches=c.batches, want_degrees=True)
    assert info.tolist() == [c.e, 0] and torch.equal(deg.cpu(), counts)
    assert_is_the_oracle_list(c, nb, ends)
    # a cap of 4: the uncapped degrees, the capped offsets, and only edges of the oracle -- those the selection rule
    # (include/se3conv_capped.h) picks from the sample's full hit set
    nb4, ends4, info4, deg4 = amd.ops.ball_query_capped(*c.args(), 4, 1234, capacity=n_dst * 4, n_batches=c.batches, want_degrees=True)
    e4 = int(torch.clamp(counts, max=4).sum())
    assert info4.tolist() == [e4, 0] and torch.equal(deg4.cpu(), counts)
    assert torch.equal(ends4.cpu(), torch.cumsum(torch.clamp(counts, max=4), 0).to(torch.int32))
    assert bool(B.has_edges(c.ref_nb, nb4[:e4], c.ps.shape[0]).all())
    want, want_ends, _ = select_capped(c.ref_nb, c.ref_ends, 4, 1234)
    assert torch.equal(canon_edges(nb4[:e4]), canon_edges(want)) and torch.equal(ends4.cpu(), want_ends)


@pytest.mark.parametrize("name", ["all_pairs_2048", "grid_32bit_1_batch", "grid_32bit_2_batches", "grid_64bit_3_batches"])
def test_self_cloud_list_is_symmetric_and_its_sources_are_the_transpose(amd, name):
    """A cloud against itself: both directions of every planted pair, and the dense `sources` output -- which backward
    takes as the source-major list, with `ends` as its offsets -- equals the transposed list group by group."""
    c = case(name)
    n = c.ps.shape[0]
    nb, ends, info, sources = amd.ops.ball_query_bounded(*c.args(), capacity=c.e, n_batches=c.batches, want_sources=True)
    assert info.tolist() == [c.e, 0]
    got = nb.cpu().to(torch.int64)
    assert bool(B.has_edges(got, c.planted, n).all()) and bool(B.has_edges(got, c.planted.flip(1), n).all())
    assert torch.equal(canon_edges(got), canon_edges(got.flip(1)))
    t_samples, t_ends = amd.ops.csr_transpose(nb, n)
    assert torch.equal(t_ends, ends)
    group = got[:, 0]                                          # (sample-major rows: row i lies in group nb[i, 0])
    assert torch.equal(torch.sort(group * n + sources.cpu().to(torch.int64)).values,
                       torch.sort(group * n + t_samples.cpu().to(torch.int64)).values)
