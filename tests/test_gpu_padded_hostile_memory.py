"""GPU: the entry points of include/se3conv_padded.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_bounded_levels_hostile_memory.py: the clouds, every output and the workspace (sized to exactly the
query's value) come from an arena, so the absent rows of a cloud hold the arena's fill (NaN points, batch id -1); no band
byte changes, the results are those of the calls on the present rows alone whatever the workspace held, every output byte is
a result or a stated pad, and the entry points are proven to have been called."""
import pytest
import torch

import hostile_memory
from conftest import canon_edges
from hostile_memory import Arena, in_arena
from padded_cases import DEV, IDENTITY, seeded_cloud

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_padded.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_batch_aabb_padded": ["test_boxes_and_ball_query", "test_knn_and_frames"],
    "se3_ball_query_padded_workspace_bytes": ["test_boxes_and_ball_query"],
    "se3_ball_query_padded": ["test_boxes_and_ball_query"],
    "se3_knn_grid_params_padded": ["test_knn_and_frames"],
    "se3_knn_query_padded_workspace_bytes": ["test_knn_and_frames"],
    "se3_knn_query_padded": ["test_knn_and_frames"],
    "se3_pca_frames_padded": ["test_knn_and_frames"],
}
# (rows_src, valid_src, rows_dst, valid_dst, batches, radius): the all-pairs and the grid path of the ball query
BALL = [(300, 171, 500, 333, 2, 0.2), (2600, 2100, 900, 640, 1, 0.12)]
# (rows, valid, k, batches): the all-pairs and the cell-grid search of the k-NN
KNN = [(700, 450, 8, 2), (9000, 5000, 16, 3)]


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(scope="module")
def want(ops):
    """The clouds and the results on the present rows alone, from the ordinary allocator: built once, left unchanged."""
    ball = []
    for i, (rs, vs, rd, vd, nb, r) in enumerate(BALL):
        ps, bs = seeded_cloud(vs, nb, 10 + i)
        pd, bd = seeded_cloud(vd, nb, 20 + i)
        ps, bs, pd, bd = (t.to(DEV) for t in (ps, bs, pd, bd))
        nbr, ends = ops.ball_query(ps, pd, bs, bd, r, nb)
        assert nbr.shape[0] > 0
        ball.append((ps, bs, pd, bd, nbr.cpu(), ends, ops.batch_aabb(ps, bs, nb)))
    knn = []
    for i, (rows, valid, k, nb) in enumerate(KNN):
        p, b = seeded_cloud(valid, nb, 30 + i)
        p, b = p.to(DEV), b.to(DEV)
        ids = ops.knn_query(p, b, k, nb)
        knn.append((p, b, ids, ops.pca_frames(p, ids, None), ops.pca_frames(p, ids, 2)))
    return ball, knn


def guarded(request, workspace_fill):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=True)


across_fills = hostile_memory.AcrossFills()


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_boxes_and_ball_query(ops, want, request, workspace_fill):
    with guarded(request, workspace_fill) as arena:
        for i, ((rs, vs, rd, vd, nb, r), (ps, bs, pd, bd, ref, ref_ends, ref_box)) in enumerate(zip(BALL, want[0])):
            p_s, b_s, p_d, b_d = in_arena(arena, ps, rs), in_arena(arena, bs, rs), in_arena(arena, pd, rd), in_arena(arena, bd, rd)
            assert torch.isnan(p_s[vs:]).all() and bool((b_d[vd:] == -1).all())
            ws_, wd_ = arena.place(torch.tensor([vs], dtype=torch.int32)), arena.place(torch.tensor([vd], dtype=torch.int32))
            mn, mx = ops.batch_aabb(p_s, b_s, nb, n_valid=ws_)
            assert torch.equal(mn, ref_box[0]) and torch.equal(mx, ref_box[1])
            e = ref.shape[0]
            cap = e + 77
            nbr, ends, info, src = ops.ball_query_padded(p_s, p_d, b_s, b_d, r, cap, nb, n_valid_src=ws_, n_valid_dst=wd_,
                                                         want_sources=True)
            assert info.tolist() == [e, 0]
            assert torch.equal(ends[:vd], ref_ends) and bool((ends[vd:] == e).all())
            assert torch.equal(canon_edges(nbr[:e]), canon_edges(ref)) and torch.equal(src[:e], nbr[:e, 1])
            # rows [E, capacity) are the stated untouched region; everything else has been written
            assert Arena.holds_fill(nbr[e:]) and Arena.holds_fill(src[e:]) and bool((nbr[:e] >= 0).all())
            across_fills(("ball", i), workspace_fill, (nbr[:e], ends, info, src[:e], mn, mx))
            # truncated: nothing past the capacity (the bands), offsets clamped
            nbr2, ends2, info2 = ops.ball_query_padded(p_s, p_d, b_s, b_d, r, e // 2, nb, n_valid_src=ws_, n_valid_dst=wd_)
            assert info2.tolist() == [e, 1] and torch.equal(nbr2, nbr[:e // 2])
            assert torch.equal(ends2, torch.clamp(ends, max=e // 2))


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_knn_and_frames(ops, want, request, workspace_fill):
    with guarded(request, workspace_fill) as arena:
        for i, ((rows, valid, k, nb), (p, b, ref_ids, ref_free, ref_fixed)) in enumerate(zip(KNN, want[1])):
            pp, bb = in_arena(arena, p, rows), in_arena(arena, b, rows)
            w = arena.place(torch.tensor([valid], dtype=torch.int32))
            ids = ops.knn_query(pp, bb, k, nb, n_valid=w)          # (9000 rows: boxes, grid parameters and the cell search)
            assert torch.equal(ids[:valid], ref_ids) and bool((ids[valid:] == -1).all())
            for axis, ref in ((None, ref_free), (2, ref_fixed)):
                fr = ops.pca_frames(pp, ids, axis, n_valid=w)
                assert torch.equal(fr[:valid].view(torch.int32), ref.view(torch.int32))
                assert torch.equal(fr[valid:], IDENTITY.to(DEV).expand(rows - valid, fr.shape[1], 9))
                across_fills(("frames", i, axis), workspace_fill, (ids, fr))
        # the all-pairs search is also asked for on the large cloud, and the grid search on its own boxes
        rows, valid, k, nb = KNN[1]
        p, b, ref_ids = want[1][1][:3]
        pp, bb = in_arena(arena, p, rows), in_arena(arena, b, rows)
        w = arena.place(torch.tensor([valid], dtype=torch.int32))
        assert torch.equal(ops.knn_query(pp, bb, k, nb, method="scan", n_valid=w)[:valid], ref_ids)
        box = ops.batch_aabb(pp, bb, nb, n_valid=w)
        assert torch.equal(ops.knn_query(pp, bb, k, nb, method="grid", box=box, n_valid=w)[:valid], ref_ids)
