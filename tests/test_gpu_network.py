"""A small encoder-decoder built the way the reference's FPNSegUNet uses the layer (models/FPNSegUNet.py:180-330):
same-level convs, strided down-convs between hierarchy levels, up-convs back, linear skips, frame pooling at the
end -- one optimiser step end to end on the GPU.  Checks the module interface under real use (several neighbourhoods,
input cloud != output cloud, geometry caches, parameters shared across calls), not the numerics of one op:
the two arithmetic modes of the library must agree with each other on the whole network, gradients must be
finite and the step must reduce the loss."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class MiniUNet(torch.nn.Module):
    def __init__(self, amd, c_in, widths, n_classes):
        super().__init__()
        f = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu")
        self.enc_same = torch.nn.ModuleList([f.create_conv_layer(c_in if i == 0 else w, w) for i, w in enumerate(widths)])
        self.enc_down = torch.nn.ModuleList([f.create_conv_layer(widths[i], widths[i + 1]) for i in range(len(widths) - 1)])
        self.dec_up = torch.nn.ModuleList([f.create_conv_layer(widths[i + 1], widths[i]) for i in range(len(widths) - 1)])
        self.skip = torch.nn.ModuleList([torch.nn.Linear(w, w) for w in widths[:-1]])
        self.head = torch.nn.Linear(widths[0], n_classes)
        self.factory = f

    def forward(self, hier, radii, x):
        feats = []
        n_lv = len(self.enc_same)
        for lv in range(n_lv):
            nb = hier.create_neighborhood(lv, lv, "ball_query", bq_radius=radii[lv])
            x = torch.nn.functional.gelu(self.enc_same[lv](p_pc_in=hier.pcs_[lv], p_pc_out=hier.pcs_[lv], p_in_features=x,
                                                           p_neighborhood=nb))
            feats.append(x)
            if lv + 1 < n_lv:
                nb = hier.create_neighborhood(lv, lv + 1, "ball_query", bq_radius=radii[lv + 1])
                x = torch.nn.functional.gelu(self.enc_down[lv](p_pc_in=hier.pcs_[lv], p_pc_out=hier.pcs_[lv + 1],
                                                               p_in_features=x, p_neighborhood=nb))
        for lv in range(n_lv - 2, -1, -1):
            nb = hier.create_neighborhood(lv + 1, lv, "ball_query", bq_radius=radii[lv + 1])
            up = self.dec_up[lv](p_pc_in=hier.pcs_[lv + 1], p_pc_out=hier.pcs_[lv], p_in_features=x, p_neighborhood=nb)
            x = torch.nn.functional.gelu(up + self.skip[lv](feats[lv]))
        return self.head(hier.pcs_[0].feature_pooling(x, "avg"))


def _setup(amd, seed):
    torch.manual_seed(seed)
    n_el, nb = 3000, 2
    pts = torch.rand(n_el * nb, 3, device=DEV)
    bid = torch.arange(nb, device=DEV, dtype=torch.int32).repeat_interleave(n_el)
    pc = amd.pc.PointcloudRotEquiv(pts, bid, {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "knn",
                                              "neigh_kwargs": {"neigh_k": 16}})
    cells = [0.08, 0.16]
    hier = amd.pc.PointHierarchyRotEquiv(pc, 2, "grid_avg", grid_radii=cells)
    radii = [0.08, 0.16, 0.32]
    return hier, radii


def _run(amd, precision, steps):
    amd.set_precision(precision)
    hier, radii = _setup(amd, 5)
    torch.manual_seed(7)
    net = MiniUNet(amd, 3, [32, 64, 96], 5).to(DEV)
    # converged EMA buffers as the pre-process pass would leave them
    for m in net.modules():
        if isinstance(m, amd.PNEConvLayerRotEquiv):
            m.norm_neigh_dist_.fill_(4.0)
            m.norm_num_neighs_.fill_(0.05)
    x = torch.randn(hier.pcs_[0].pts_.shape[0] * 2, 3, device=DEV)
    labels = torch.randint(0, 5, (hier.pcs_[0].pts_.shape[0],), device=DEV)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    losses, out0, g0 = [], None, None
    for it in range(steps):
        opt.zero_grad()
        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        out = net(hier, radii, x)
        loss = torch.nn.functional.cross_entropy(out, labels)
        loss.backward()
        if it == 0:
            out0 = out.detach().clone()
            g0 = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
        opt.step()
        losses.append(float(loss.detach()))
    return out0, g0, losses


def test_mini_unet_training_step(built_library):
    import se3conv3d_amd as amd

    prev = amd.get_precision()
    try:
        out_a, g_a, losses = _run(amd, "bf16x3", 4)
        out_b, g_b, _ = _run(amd, "fp32", 1)
    finally:
        amd.set_precision(prev)
    assert torch.isfinite(out_a).all() and torch.isfinite(g_a).all()
    assert losses[-1] < losses[0], losses
    # the two arithmetic modes of the library agree on the whole network (9 convs deep, forward and backward)
    assert float((out_a - out_b).norm() / out_b.norm()) < 2e-4
    assert float((g_a - g_b).norm() / g_b.norm()) < 2e-4


def test_reference_resnetformer_block_runs_unchanged(built_library):
    """The reference's ResNetFormer block (tests/golden/resnetformer_block.npz: its state_dict, input, output and all
    gradients from the reference's own Python) rebuilt from se3conv3d_amd parts: the state_dict loads key for key and
    the block reproduces output, input gradient, parameter gradients and batch-norm statistics in both arithmetic
    modes."""
    import os
    import numpy as np
    import se3conv3d_amd as amd
    from conftest import GOLDEN, rel_err

    d = np.load(os.path.join(GOLDEN, "resnetformer_block.npz"))
    t = lambda k: torch.from_numpy(np.asarray(d[k])).to(DEV)
    pc = amd.pc.PointcloudRotEquiv.from_frames(t("pts"), t("batch"), t("frames"))
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]))
    for precision, tol in (("fp32", 5e-6), ("bf16x3", 5e-5), ("bf16x3_t16", 5e-5)):
        amd.set_precision(precision)
        blk = amd.ResNetFormer(32, 48, amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu"), amd.BatchNormPC, 0.0).to(DEV)
        state = {k[len("state/"):]: t(k) for k in d.files if k.startswith("state/")}
        res = blk.load_state_dict(state, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        blk.train()
        x = t("x").requires_grad_(True)
        out = blk(pc, x, nbh)
        out.backward(t("g"))
        assert rel_err(out, t("out")) < tol and rel_err(x.grad, t("dx")) < tol
        for name, p in blk.named_parameters():
            assert rel_err(p.grad, t("grad/" + name)) < 4 * tol, (precision, name)
        for k, v in blk.state_dict().items():
            if "running" in k:
                np.testing.assert_allclose(v.cpu().numpy(), d["after/" + k], rtol=1e-4, atol=1e-5)
    amd.set_precision("bf16x3")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("workload", ["headline", "scannet150k_f1"])
def test_bench_two_ranks_on_one_gpu_rehearsal(workload):
    """`bench.py --gpus 2` started plainly forks two ranks (torch.distributed.run children); with --share-gpu both use
    this box's one GPU and gloo carries the barrier / MAX reduce / result gather: the whole N-rank path runs real
    kernels -- two scenes (seeds = scene ids), one JSON line from rank 0 with n_gpus = 2 and both checksums.
    `scannet150k_f1` is the workload BASELINE.json's config 5 names (150 k-point scenes sharded by scene, F = 1)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-gpu", "--steps", "3",
                        "--warmup", "1", "--full", "--no-cpu-baseline", "--workload", workload],
                       capture_output=True, text=True, timeout=550, env=env, cwd=root)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and sorted(rec["scene_checksums"]) == ["0", "1"]
    assert rec["scene_checksums"]["0"] != rec["scene_checksums"]["1"]      # different scenes per rank
    assert "roofline" not in rec                                            # single-GPU extras stay out of N > 1 lines
    assert rec["config"]["workload"].startswith(workload) and rec["config"]["n_points"] == (65536 if workload == "headline" else 150000)


@pytest.mark.timeout(600)
def test_bench_rccl_path_with_one_rank():
    """The N-rank code path of bench.py on the one GPU of this box: a one-rank RCCL process group (init with the device,
    barrier, MAX / SUM all-reduce of the timing on the GPU, tensor all-gather of the checksums) and the step captured
    into a HIP graph while the communicator and its watchdog thread are alive."""
    import json
    import os
    import socket
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               SE3_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-fp32"], capture_output=True, text=True, timeout=550, env=env, cwd=root)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 1 and rec["value"] > 0 and list(rec["scene_checksums"]) == ["0"]
    assert rec["config"]["launch"].startswith("hipGraph"), rec["config"]["launch"]
    # the level-to-level convolutions (bounded ball query + transposition + forward + backward as ONE captured graph) replay
    # next to the communicator too: in round 4 they faulted there -- memset nodes of rocPRIM's one-sweep sort
    legs = rec["down_up"]["headline"]
    assert {legs["down"]["launch"], legs["up"]["launch"]} == {"hipGraph replay"}, legs


@pytest.mark.timeout(600)
def test_bench_plain_run_dumps_the_timed_outputs(built_library, tmp_path):
    """A plain `bench.py` run: the headline keys only (no leg of --full), `--steps` timed steps, and `--dump-outputs`
    writes what the step computed -- float32 files inside the size budget, the arrays that fit whole equal to the same
    seeded stack computed again in this process."""
    import json
    import os
    import subprocess
    import sys

    import numpy as np

    import bench
    import se3conv3d_amd as amd
    from conftest import rel_err
    from se3conv3d_amd import workloads as W

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=550, env=env, cwd=root)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 4 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["higher_is_better"] is True
    assert rec["unit"] == "Mpoints/s" and rec["dtype"].startswith("bf16x3")
    assert not {"roofline", "single_layer", "cpu_baseline", "scene_checksums", "fp32_mode"} & set(rec)

    files = sorted(os.listdir(tmp_path))
    assert len(files) == 4 * 5 and sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 10 ** 6
    amd.set_precision("bf16x3")
    levels = W.build_stack(W.WORKLOADS["headline"], torch.device(DEV), seed=0)
    bench.step(levels)
    whole = 0
    for name, t in bench.step_outputs(levels).items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and np.isfinite(got).all(), name
        if got.shape == tuple(t.shape):
            whole += 1
            assert rel_err(torch.from_numpy(got), t) < 1e-5, name
        else:  # a seeded sample of the rows
            assert got.shape[1:] == tuple(t.shape[1:]) and 0 < got.shape[0] < t.shape[0], name
    assert whole >= 4 * 3  # at least every parameter gradient is written whole
