"""`-m gpu`: point-cloud kernels (FPS, kNN, fused set abstraction, vector attention, SceneMapEncoder)
vs the reference goldens and the CPU oracle.  Indices are bit-exact; float outputs: report() keeps the absolute bars (2e-4 ... 3e-4), the
bound that bites is report_f32_class (tests/gpu_util.py): the HIP error against the float64 twin of the oracle (same FPS / kNN picks,
asserted) is at most 4 x the float32 reference's own error against that twin, plus one float32 ulp of the largest output."""
import pytest
import torch

from afm import pointops, synth
from afm import scene as S
from conftest import golden
from gpu_util import dev, grad_forms, load_named_weights, report, report_f32_class, to_f64, write_parity_table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,n,m", [(2, 200, 50), (3, 512, 128), (2, 2048, 512), (2, 8192, 2048), (1, 8192, 1024), (2, 100, 100), (1, 64, 1),
                                   (2, 3000, 700), (1, 1536, 100), (3, 5000, 1250), (1, 8192, 8192), (2, 2049, 40), (1, 4096, 31)])
def test_fps_bit_exact(B, n, m):
    from oracle import pointops_ref as po
    p = synth.scene_cloud(B, n, seed=21).reshape(B * n, 3)
    o = torch.arange(1, B + 1, dtype=torch.int32) * n
    no = torch.arange(1, B + 1, dtype=torch.int32) * m
    want = po.furthest_sampling(p, o, no)
    got = pointops.furthest_point_sampling(p.to(dev()), B, n, m).cpu()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} indices differ"


_FPS_EDGES = [64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1535, 1536, 2048, 2049, 4096, 4097, 8192, 8193, 12800, 12801, 16384]


@pytest.mark.parametrize("n,m", [(n, min(n, 40)) for n in _FPS_EDGES] + [(1536, 31), (16384, 2)])
def test_fps_on_both_sides_of_every_dispatch_boundary(n, m):
    """csrc/fps_plan.h changes kernel between n and n + 1 at each of these sizes (tests/test_fps_plan_host.py pins the rule itself); at
    n = 1536 also between m = 31 (plain kernel) and m = 32 (pruned).  12800 < n <= 16384 is the only range of the kernel that reads the winner's
    coordinates from global memory (12 n bytes exceed the LDS budget): 12801, 16384, and (16384, 2) as its shortest run.
    Two samples, so the second one's row offset is exercised.  Bit-exact against the oracle."""
    from oracle import pointops_ref as po
    B = 2
    p = synth.scene_cloud(B, n, seed=29).reshape(B * n, 3)
    want = po.furthest_sampling(p, torch.tensor([n, 2 * n], dtype=torch.int32), torch.tensor([m, 2 * m], dtype=torch.int32))
    got = pointops.furthest_point_sampling(p.to(dev()), B, n, m).cpu()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} indices differ"


def test_fps_refuses_more_than_16384_points():
    """include/afm_hip.h: n <= 16384.  The refusal (AFM_E_UNSUPPORTED) is returned before any launch."""
    from afm import ffi
    p = torch.zeros(16385, 3, device=dev())
    with pytest.raises(ffi.AfmError, match="afm_fps failed: unsupported shape"):
        pointops.furthest_point_sampling(p, 1, 16385, 2)


def test_fps_ties_pick_lowest_index():
    # duplicated points (real chunks contain them, prepare/generate_contact_data.py:418-423): ties -> lowest index
    from oracle import pointops_ref as po
    base = synth.scene_cloud(1, 64, seed=22).reshape(64, 3)
    p = torch.cat([base, base], 0).contiguous()                      # every point twice, one sample of 128
    o, no = torch.tensor([128], dtype=torch.int32), torch.tensor([32], dtype=torch.int32)
    want = po.furthest_sampling(p, o, no)
    got = pointops.furthest_point_sampling(p.to(dev()), 1, 128, 32).cpu()
    assert torch.equal(got, want) and got.max() < 64


@pytest.mark.parametrize("n,shift,m", [(8192, 70, 600), (2048, 33, 300), (512, 1, 256), (4096, 17, 3000), (8192, 4097, 8192)])
def test_fps_ties_across_lanes_and_waves(n, shift, m):
    """Every point twice, the copies `shift` rows apart: the two holders of every maximum sit in different lanes and (n = 8192: 4 waves,
    n = 2048: 1 wave of 32-point threads) different waves, so each round exercises the tie paths of the wave-level and of the workgroup-level
    arg-max (ballot with more than one holder -> lowest index).  m above the number of DISTINCT points (round 6: 3000 of 2048, 8192 of 4096) runs
    the rounds in which every remaining minimum is zero: all wave keys tie at distance 0, no box test of fps_pruned_kernel asks for a scan
    (no lower bound is below a maximum of 0), and the pick is the lowest index of the sample, round after round.  Bit-exact against the oracle."""
    from oracle import pointops_ref as po
    base = synth.scene_cloud(1, n // 2, seed=27).reshape(n // 2, 3)
    p = torch.cat([base, base.roll(shift, 0)], 0).contiguous()
    o, no = torch.tensor([n], dtype=torch.int32), torch.tensor([m], dtype=torch.int32)
    want = po.furthest_sampling(p, o, no)
    got = pointops.furthest_point_sampling(p.to(dev()), 1, n, m).cpu()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {m} indices differ"
    both = torch.cat([p, p.flip(0)], 0).contiguous()              # two samples in one launch, the second with the copies in reverse order
    want2 = po.furthest_sampling(both, torch.tensor([n, 2 * n], dtype=torch.int32), torch.tensor([m, 2 * m], dtype=torch.int32))
    got2 = pointops.furthest_point_sampling(both.to(dev()), 2, n, m).cpu()
    assert torch.equal(got2, want2)


@pytest.mark.parametrize("k,B,n,m", [(8, 2, 300, 300), (16, 2, 2048, 512), (16, 2, 8192, 2048), (8, 1, 8192, 8192), (3, 2, 128, 512), (16, 1, 16, 16)])
def test_knn_bit_exact(k, B, n, m):
    from oracle import pointops_ref as po
    p = synth.scene_cloud(B, n, seed=23).reshape(B * n, 3)
    q = p if m == n else synth.scene_cloud(B, m, seed=24).reshape(B * m, 3)
    o = torch.arange(1, B + 1, dtype=torch.int32) * n
    no = torch.arange(1, B + 1, dtype=torch.int32) * m
    wi, wd = po.knn_query(k, p, q, o, no)
    gi, gd = pointops.knn(k, p.to(dev()), q.to(dev()), B, n, m)
    assert torch.equal(gi.cpu(), wi), f"{(gi.cpu() != wi).sum().item()} of {wi.numel()} indices differ"
    assert torch.equal(gd.cpu(), wd)


@pytest.mark.parametrize("k,B,n,m,dup", [(8, 2, 8192, 8192, False), (16, 2, 8192, 8192, True), (3, 1, 4096, 8192, False), (16, 3, 5000, 5000, False),
                                         (8, 1, 4100, 4100, True), (16, 2, 8192, 2048, False), (3, 2, 2048, 8192, False)])
def test_knn_pruned_equals_plain_kernel_and_oracle(k, B, n, m, dup):
    """Round 6: afm_knn_ws - Morton-sorted candidate tiles with bounding boxes, wave-level skipping, the k best as (distance bits, index) keys -
    against the plain all-pairs kernel (afm_knn) bit for bit, indices AND distances, and against the oracle: ragged tile counts (n = 5000, 4100), more
    queries than candidates, self-search, shapes the pruned form does not take (they fall through to the plain kernel), and DUPLICATED points (every point twice, copies far apart in index: ties in d2 must
    come out in index order although the tiles are not visited in index order)."""
    from oracle import pointops_ref as po
    p = synth.scene_cloud(B, n, seed=31).reshape(B * n, 3)
    if dup:
        h = n // 2
        p = p.view(B, n, 3).clone()
        p[:, h:2 * h] = p[:, :h].roll(17, 1)
        p = p.reshape(B * n, 3).contiguous()
    q = p if m == n else (p.view(B, n, 3)[:, torch.randperm(n, generator=torch.Generator().manual_seed(5))[:m]].reshape(B * m, 3).contiguous() if dup and m <= n
                          else synth.scene_cloud(B, m, seed=32).reshape(B * m, 3))
    pd, qd = p.to(dev()), (None if m == n else q.to(dev()))
    qd = pd if qd is None else qd
    assert pointops.PRUNED_KNN
    gi, gd = pointops.knn(k, pd, qd, B, n, m)
    pointops.PRUNED_KNN = False
    try:
        pi, pdist = pointops.knn(k, pd, qd, B, n, m)
    finally:
        pointops.PRUNED_KNN = True
    assert torch.equal(gi, pi), f"{(gi != pi).sum().item()} of {gi.numel()} indices differ from the plain kernel"
    assert torch.equal(gd, pdist)
    o = torch.arange(1, B + 1, dtype=torch.int32) * n
    no = torch.arange(1, B + 1, dtype=torch.int32) * m
    wi, wd = po.knn_query(k, p, q, o, no)
    assert torch.equal(gi.cpu(), wi) and torch.equal(gd.cpu(), wd)


@pytest.mark.parametrize("stride", [4, 8])
def test_transition_down_vs_reference_golden(stride):
    g = golden(f"transition_down_s{stride}")
    td = load_named_weights(S.TransitionDown(32, 64, stride=stride, nsample=16)).to(dev()).eval()
    n_p, y = td.run(g["p"].to(dev()), g["x"].to(dev()), 2)
    assert torch.equal(n_p.cpu(), g["n_p"])
    report(f"TransitionDown stride {stride}", y, g["y"], 2e-4)
    from oracle import scene_ref as sr, shapes as sh
    sd = {"td." + k: v for k, v in sh.weights(sh.transition_down("", 32, 64, stride)).items()}
    p64, y64, _, _ = sr.transition_down(to_f64(sd), "td", g["p"].double(), g["x"].double(), g["o"], stride, 16)
    assert torch.equal(p64.float(), g["n_p"])                           # the float64 run sampled the reference's coordinates
    report_f32_class(f"TransitionDown stride {stride}", y, g["y"], y64, 2e-4)


def test_transition_down_stride1_vs_reference_golden():
    g = golden("transition_down_s1")
    td = load_named_weights(S.TransitionDown(9, 32, stride=1, nsample=8)).to(dev()).eval()
    _, y = td.run(torch.zeros(512, 3, device=dev()), g["x"].to(dev()), 2)
    report("TransitionDown stride 1", y, g["y"], 2e-4)
    from oracle import scene_ref as sr, shapes as sh
    sd = {"td." + k: v for k, v in sh.weights(sh.transition_down("", 9, 32, 1)).items()}
    report_f32_class("TransitionDown stride 1", y, g["y"], sr.transition_down(to_f64(sd), "td", None, g["x"].double(), None, 1, 8)[1], 2e-4)


@pytest.mark.parametrize("c,k", [(32, 8), (64, 16)])
def test_point_transformer_block_vs_reference_golden(c, k):
    g = golden(f"pt_block_c{c}_k{k}")
    blk = load_named_weights(S.PointTransformerBlock(c, c, 8, nsample=k)).to(dev()).eval()
    p, x = g["p"].to(dev()), g["x"].to(dev())
    knn_idx, _ = pointops.knn(k, p, p, 2, 128, 128)
    lay, y = blk.transformer2.run(p, x, knn_idx), blk.run(p, x, knn_idx)
    report(f"PointTransformerLayer c{c} k{k}", lay, g["layer_out"], 2e-4)
    report(f"PointTransformerBlock c{c} k{k}", y, g["y"], 2e-4)
    from oracle import pointops_ref as po, scene_ref as sr, shapes as sh
    assert torch.equal(knn_idx.cpu(), po.knn_query(k, g["p"], g["p"], g["o"], g["o"])[0])          # the neighbours both oracle runs use
    sd64 = to_f64({"b." + kk: v for kk, v in sh.weights(sh.pt_block("", c)).items()})
    report_f32_class(f"PointTransformerLayer c{c} k{k}", lay, g["layer_out"],
                     sr.point_transformer_layer(sd64, "b.transformer2", g["p"].double(), g["x"].double(), g["o"], k), 2e-4)
    report_f32_class(f"PointTransformerBlock c{c} k{k}", y, g["y"], sr.point_transformer_block(sd64, "b", g["p"].double(), g["x"].double(), g["o"], k), 2e-4)


@pytest.mark.parametrize("c,k,n", [(128, 16, 256), (256, 16, 64)])
def test_point_transformer_block_wide_vs_oracle(c, k, n):
    from oracle import scene_ref as sr, shapes as sh
    sd = {"b." + kk: v for kk, v in sh.weights(sh.pt_block("", c)).items()}
    blk = load_named_weights(S.PointTransformerBlock(c, c, 8, nsample=k)).to(dev()).eval()
    p = synth.scene_cloud(2, n, seed=31).reshape(2 * n, 3); x = synth.gaussian("ptw_x", (2 * n, c))
    o = torch.tensor([n, 2 * n], dtype=torch.int32)
    want = sr.point_transformer_block(sd, "b", p, x, o, k)
    knn_idx, _ = pointops.knn(k, p.to(dev()), p.to(dev()), 2, n, n)
    got = blk.run(p.to(dev()), x.to(dev()), knn_idx)
    report(f"PointTransformerBlock c{c}", got, want, 3e-4)
    report_f32_class(f"PointTransformerBlock c{c}", got, want, sr.point_transformer_block(to_f64(sd), "b", p.double(), x.double(), o, k), 3e-4)


def _same_path(a32, a64):
    """The float32 and the float64 oracle run of a SceneMapEncoder picked the same points and neighbours at every level."""
    for l32, l64 in zip(a32, a64):
        assert torch.equal(l32["p"], l64["p"].float()) and torch.equal(l32["self_knn_idx"], l64["self_knn_idx"])
        if "fps_idx" in l32:
            assert torch.equal(l32["fps_idx"], l64["fps_idx"]) and torch.equal(l32["knn_idx"], l64["knn_idx"])


def _encoder64(sr, sd, pre, xyz, contact, **kw):
    """Float64 twin of sr.scene_map_encoder, after checking that it walks the float32 run's discrete path."""
    _, a32 = sr.scene_map_encoder(sd, pre, xyz, contact, return_aux=True, **kw)
    out64, a64 = sr.scene_map_encoder(to_f64(sd), pre, xyz.double(), contact.double(), return_aux=True, **kw)
    _same_path(a32, a64)
    return out64


def test_scene_map_encoder_vs_reference_golden():
    g = golden("scene_map_encoder_N1024")
    enc = load_named_weights(S.SceneMapEncoder(6, [32, 64, 128, 256], [2, 2, 2, 2], num_points=1024)).to(dev()).eval()
    from oracle import scene_ref as sr, shapes as sh
    want64 = _encoder64(sr, sh.weights(sh.scene_map_encoder("")), "", g["xyz"], g["contact"])
    for form, got in grad_forms(lambda: enc(g["xyz"].to(dev()), g["contact"].to(dev()))):
        report("SceneMapEncoder N=1024" + form, got, g["out"], 3e-4)
        report_f32_class("SceneMapEncoder N=1024" + form, got, g["out"], want64, 3e-4)


def test_set_abstraction_full_size_vs_oracle():
    """BASELINE config [3]: N = 8192 -> 2048 (faithful stride 4) and -> 1024 (stride 8), vs the CPU oracle."""
    from oracle import scene_ref as sr, shapes as sh
    B, n = 2, 8192
    p = synth.scene_cloud(B, n, seed=41).reshape(B * n, 3); x = synth.gaussian("sa_x", (B * n, 32))
    o = torch.arange(1, B + 1, dtype=torch.int32) * n
    for stride in (4, 8):
        sd = {"td." + k: v for k, v in sh.weights(sh.transition_down("", 32, 64, stride)).items()}
        wp, wy, _, aux = sr.transition_down(sd, "td", p, x, o, stride, 16)
        td = load_named_weights(S.TransitionDown(32, 64, stride=stride, nsample=16)).to(dev()).eval()
        n_p, y = td.run(p.to(dev()), x.to(dev()), B)
        assert torch.equal(n_p.cpu(), wp)
        report(f"set abstraction 8192->{n // stride}", y, wy, 2e-4)
        p64, y64, _, aux64 = sr.transition_down(to_f64(sd), "td", p.double(), x.double(), o, stride, 16)
        assert torch.equal(p64.float(), wp) and torch.equal(aux64["fps_idx"], aux["fps_idx"]) and torch.equal(aux64["knn_idx"], aux["knn_idx"])
        report_f32_class(f"set abstraction 8192->{n // stride}", y, wy, y64, 2e-4)


def test_point_transformer_seg_vs_reference_golden():
    """Frozen scene backbone of the HUMANISE / novel ADM: 5-level encoder + FPN decoder (TransitionUp, 3-NN interpolation)."""
    g = golden("point_transformer_seg_N4096")
    seg = load_named_weights(S.PointTransformerSeg(c=6, num_points=4096)).to(dev()).eval()
    from oracle import scene_ref as sr, shapes as sh
    # (FPS / kNN read the float32 coordinates in both runs - oracle/pointops_ref.py - and point_transformer_seg exposes no indices)
    out64 = sr.point_transformer_seg(to_f64(sh.weights(sh.point_transformer_seg(""))), "", g["xyz"].double(), g["color"].double())[0]
    for form, res in grad_forms(lambda: seg((g["xyz"].to(dev()), g["color"].to(dev())))):
        out = res[0].cpu()
        report("PointTransformerSeg N=4096 (sampled rows)" + form, out[g["rows"].long()], g["out_rows"], 3e-4)
        report_f32_class("PointTransformerSeg N=4096 (sampled rows)" + form, out[g["rows"].long()], g["out_rows"], out64[g["rows"].long()], 3e-4)
        assert abs(out.double().sum().item() - float(g["out_sum"])) < 1e-2 * max(1.0, abs(float(g["out_abs_sum"])) * 1e-3)


def test_cdm_with_scene_backbone_vs_oracle():
    """ts2m_contact-style CDM: frozen PointTransformerSeg(c=6) features (32-d) feed the Perceiver (41 input channels)."""
    from afm.base import create_model
    from oracle import denoiser_ref as dr, scene_ref as sr, shapes as sh
    from test_gpu_cdm import cdm_cfg
    cfg = cdm_cfg(num_points=4096, point_feats=True)
    cfg.model.scene_model.use_openscene = False
    cfg.model.scene_model.use_color = True
    m = create_model(cfg, device=dev())
    load_named_weights(m)
    m = m.to(dev()).eval()
    B, N = 1, 4096
    x = synth.gaussian("cdmseg_x", (B, N, 6)); xyz = synth.scene_cloud(B, N, seed=71); col = synth.contact_map(B, N, joints=3, seed=71)
    text = synth.text_feature(B); t = torch.tensor([123])
    sd_seg = {k[len("scene_model."):]: v for k, v in sh.weights({"scene_model." + k: v for k, v in sh.point_transformer_seg("", c=6).items()}).items()}
    emb = sr.point_transformer_seg(sd_seg, "", xyz, col)
    want = dr.cdm_forward(sh.weights(sh.cdm(point_feat_dim=32)), x, t, text, xyz, pc_emb=emb)
    emb64 = sr.point_transformer_seg(to_f64(sd_seg), "", xyz.double(), col.double())
    want64 = dr.cdm_forward(to_f64(sh.weights(sh.cdm(point_feat_dim=32))), x.double(), t, text.double(), xyz.double(), pc_emb=emb64)
    for form, got in grad_forms(lambda: m(x.to(dev()), t.to(dev()), c_text_feat=text.to(dev()), c_pc_xyz=xyz.to(dev()), c_pc_feat=col.to(dev()))):
        report("CDM + frozen scene backbone vs oracle" + form, got, want, 3e-4)
        report_f32_class("CDM + frozen scene backbone vs oracle" + form, got, want, want64, 3e-4)


def test_scene_map_encoder_full_size_vs_oracle():
    """VERDICT r1 #4b: the WHOLE SceneMapEncoder (models/modules.py:124-167) at the shape t2m_contact_motion really runs - N = 8192 points,
    planes [32, 64, 128, 256], strides [1, 4, 4, 4] -> 128 groups of 256 channels - HIP path vs the CPU oracle, one sample
    (FPS 8192 -> 2048 -> 512 -> 128, 11 kNN calls, 4 set abstractions, 8 vector-attention blocks)."""
    from afm import scene as S
    from oracle import scene_ref as sr, shapes as sh
    enc = S.SceneMapEncoder(point_feat_dim=6, planes=[32, 64, 128, 256], blocks=[2, 2, 2, 2], num_points=8192)
    sd = {k[len("contact_encoder."):]: v for k, v in sh.weights(sh.cmdm()).items() if k.startswith("contact_encoder.")}
    res = enc.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    enc = enc.to(dev()).eval()
    B, N = 1, 8192
    xyz, contact = synth.scene_cloud(B, N, seed=77), synth.contact_map(B, N, seed=77)
    want = sr.scene_map_encoder({"contact_encoder." + k: v for k, v in sd.items()}, "contact_encoder", xyz, contact, blocks=(2, 2, 2, 2))
    want64 = _encoder64(sr, {"contact_encoder." + k: v for k, v in sd.items()}, "contact_encoder", xyz, contact, blocks=(2, 2, 2, 2))
    for form, got in grad_forms(lambda: enc(xyz.to(dev()), contact.to(dev()))):
        assert got.shape == (B, 128, 256)
        report("SceneMapEncoder N=8192 vs oracle" + form, got, want, 2e-4)
        report_f32_class("SceneMapEncoder N=8192 vs oracle" + form, got, want, want64, 2e-4)
    # round 6: the inference path computes FPS / kNN of all levels on a side stream under the feature passes (the training path's geometry
    # pyramid); same kernels on the same inputs - bit-identical to the level-by-level form, also for a batch and on repeats
    xb, cb = synth.scene_cloud(3, N, seed=78).to(dev()), synth.contact_map(3, N, seed=78).to(dev())
    for grad in (True, False):                     # (the switch belongs to the inference path, which a caller reaches under torch.no_grad())
        outs = []
        with torch.set_grad_enabled(grad):
            for overlap in (True, False, True):
                enc.overlap_geometry = overlap
                outs.append(enc(xb, cb).clone())
        enc.overlap_geometry = True
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_zz_write_parity_table():
    """Not a check: stores the [parity-f32] figures measured so far (gpu_util.write_parity_table -> profiles/r07_parity_f32_class.json)."""
    write_parity_table()
