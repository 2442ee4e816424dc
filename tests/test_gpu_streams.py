"""Every native op where a trainer may issue it: a side stream, two streams at once, a fresh host thread, a second device.

Each entry point of the C ABI takes the caller's stream (_native._stream: torch's current stream on the tensors' device).  The per-op
numerics are held to float64 elsewhere; here the values already proven must not depend on WHERE the call is issued: every output and
every gradient of the side-stream run is bit-equal to the default-stream run of the same inputs (tests/streams.py: the protocol, the
decoy and the delay).  tests/test_stream_discipline.py holds the same contract statically.

test_sensitivity_* show that the harness detects what it is for: with _native._stream patched to another stream the op runs during the
delay, on the decoy.  Observed on an MI355X (and asserted): a launch on the NULL stream is not ordered behind torch's side streams
either (they are created non-blocking), so it too computes the decoy's result.

Element-wise ops come first, the rasterizer last."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import scene_synth as S
import streams as ST
from util import cov3d_from, raster_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def N():
    from diff_gaussian_rasterization import _native
    return _native


@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream(device=DEV)


def _dev(d, device):
    """{name: host tensor or array} -> the same on the device."""
    return {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(device).contiguous() for k, v in d.items()}


def _all(state):
    return [v for v in state.values() if isinstance(v, torch.Tensor)]


def _leaf(t):
    return t.detach().requires_grad_(True)           # shares the staged buffer: no copy, no launch


# ---- element-wise and per-row ops ----------------------------------------------------------------------------------------------------

def _act_make(seed, device):
    import training_ref as R
    (s, r, o), (gs, gr, go) = R.activation_inputs(1000, 100 + seed)
    return _dev(dict(s=s, r=r, o=o, gs=gs, gr=gr, go=go), device)


def _act_fwd(st):
    from diff_gaussian_rasterization import _native as N
    a = N.activations_forward(st["s"], st["r"], st["o"])
    return dict(scales=a[0], rotations=a[1], opacities=a[2])


def _act_run(st):
    from diff_gaussian_rasterization import _native as N
    out = _act_fwd(st)
    g = N.activations_backward(out["scales"], st["r"], out["opacities"], st["gs"], st["gr"], st["go"])
    return dict(out, d_scaling=g[0], d_rotation=g[1], d_opacity=g[2])


ADAM_P, ADAM_M = 4097, 16
ADAM_SHAPES = dict(xyz=(ADAM_P, 3), features=(ADAM_P, ADAM_M, 3), opacity=(ADAM_P, 1), scaling=(ADAM_P, 3), rotation=(ADAM_P, 4))


def _adam_make(sparse):
    def make(seed, device):
        from fused_adam import FusedAdam, SparseFusedAdam
        g = torch.Generator().manual_seed(200 + seed)
        params, groups = {}, []
        for i, (name, shape) in enumerate(ADAM_SHAPES.items()):
            p = torch.nn.Parameter(torch.randn(*shape, generator=g).to(device))
            p.grad = torch.randn(*shape, generator=g).to(device)
            params[name] = p
            groups.append({"params": [p], "lr": 1e-3 * (i + 1), "name": name})
        opt = (SparseFusedAdam if sparse else FusedAdam)(groups, lr=0.0, eps=1e-15)
        for p in params.values():                     # a mid-training state: no zero fill on first use
            opt.state[p]["step"] = torch.tensor(6.0)
            opt.state[p]["exp_avg"] = (0.1 * torch.randn(*p.shape, generator=g)).to(device)
            opt.state[p]["exp_avg_sq"] = ((0.03 * torch.randn(*p.shape, generator=g)) ** 2).to(device)
        mask = (torch.rand(ADAM_P, generator=g) < 0.5).to(device) if sparse else None
        return dict(params=params, opt=opt, mask=mask)
    return make


def _adam_tensors(st):
    out = []
    for p in st["params"].values():
        out += [p, p.grad, st["opt"].state[p]["exp_avg"], st["opt"].state[p]["exp_avg_sq"]]
    return out


def _adam_staged(st):
    return _adam_tensors(st) + ([st["mask"]] if st["mask"] is not None else [])


def _adam_result(st):
    out = {}
    for name, p in st["params"].items():
        out.update({name: p, name + "_m": st["opt"].state[p]["exp_avg"], name + "_v": st["opt"].state[p]["exp_avg_sq"]})
    return out


def _adam_run(st):
    if st["mask"] is None:
        st["opt"].step()
    else:
        st["opt"].step(st["mask"])
    return _adam_result(st)


def _densify_make(seed, device):
    import training_ref as R
    radii, grad, max_radii, accum, denom = R.densify_inputs(5000, 300 + seed)
    return _dev(dict(radii=radii, grad=torch.nan_to_num(grad, nan=0.25), max_radii=max_radii, accum=accum, denom=denom), device)


def _densify_run(st):
    from diff_gaussian_rasterization import _native as N
    N.densify_stats(st["radii"], st["grad"], st["max_radii"], st["accum"], st["denom"])
    return dict(max_radii=st["max_radii"], accum=st["accum"], denom=st["denom"])


def _knn_make(seed, device):
    return _dev(dict(xyz=torch.randn(777, 3, generator=torch.Generator().manual_seed(400 + seed))), device)


def _knn_run(st):
    from simple_knn._C import distCUDA2
    return dict(dist2=distCUDA2(st["xyz"]))


COMPOSE = (257, 8, 16)


def _compose_make(seed, device):
    import structured_ref as SR
    inputs, grads = SR.make_case(*COMPOSE, 500 + seed, device)
    return dict({f"in{i}": t for i, t in enumerate(inputs)}, **{f"g{i}": t for i, t in enumerate(grads)})


def _compose_run(st):
    from diff_gaussian_rasterization.structured import compose_structures
    leaves = [_leaf(st[f"in{i}"]) for i in range(5)]
    outs = compose_structures(*leaves, COMPOSE[1], COMPOSE[2], native=True)
    grads = torch.autograd.grad(outs, leaves, [st[f"g{i}"] for i in range(5)])
    return dict({f"out{i}": t for i, t in enumerate(outs)}, **{f"d{i}": t for i, t in enumerate(grads)})


def _decoder_make(shape):
    def make(seed, device):
        import decoder_ref as DR
        B, L, pos, K, M = shape                        # as tests/test_gpu_decoder.py SHAPES
        pos, latents, params, G = DR.float_case(B, L, 63 if pos else 0, K * (11 + 3 * M), 600 + seed)
        d = dict(latents=latents, G=G, **{f"p{i}": p for i, p in enumerate(params)})
        if pos is not None:
            d["pos"] = pos
        return _dev(d, device)
    return make


def _decoder_run(st):
    from diff_gaussian_rasterization.decoder import decode_structures
    leaves = [_leaf(st["latents"])] + [_leaf(st[f"p{i}"]) for i in range(6)]
    out = decode_structures(*leaves, pos_emb=st.get("pos"), native=True)
    grads = torch.autograd.grad(out, leaves, st["G"])
    return dict(decoded=out, **{f"d{i}": g for i, g in enumerate(grads)})


MCMC_P, MCMC_N = 4099, 700


def _mcmc_make(seed, device):
    import mcmc_ref as MR
    o, s = MR.relocation_inputs(MCMC_P, 700 + seed)
    xyz, s2, rot, o2, xi = MR.noise_inputs(MCMC_P, 710 + seed)
    g = torch.Generator().manual_seed(720 + seed)
    perm = torch.randperm(MCMC_P, generator=g)
    dead = perm[:MCMC_N]                                                   # disjoint from the sources
    sampled = perm[MCMC_N:][torch.randint(0, MCMC_P - MCMC_N, (MCMC_N,), generator=g)]       # with repeats
    d = dict(o=o, s=s, xyz=xyz, s2=s2, rot=rot, o2=o2, xi=xi, sampled=sampled, dead=dead, go=torch.randn(MCMC_P, 1, generator=g),
             gs=torch.randn(MCMC_P, 3, generator=g))
    for name, shape in (("xyz", (MCMC_P, 3)), ("o", (MCMC_P, 1)), ("s", (MCMC_P, 3))):
        d[name + "_m"], d[name + "_v"] = torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)
    return _dev(d, device)


def _mcmc_relocation(st):
    from diff_gaussian_rasterization import mcmc
    new_o, new_s = mcmc.compute_relocation(st["o"], st["s"], st["sampled"], 0.005, native=True)
    return dict(new_o=new_o, new_s=new_s)


def _mcmc_rows(st):
    from diff_gaussian_rasterization import mcmc
    out = _mcmc_relocation(st)
    tensors = [(st["xyz"], st["xyz_m"], st["xyz_v"], "copy"), (st["o"], st["o_m"], st["o_v"], "opacity"), (st["s"], st["s_m"], st["s_v"], "scaling")]
    mcmc.relocate_rows(tensors, st["sampled"], st["dead"], out["new_o"], out["new_s"], native=True)
    return dict(out, **{k: st[k] for k in ("xyz", "xyz_m", "xyz_v", "o", "o_m", "o_v", "s", "s_m", "s_v")})


def _mcmc_noise(st):
    from diff_gaussian_rasterization import mcmc
    mcmc.inject_position_noise(st["xyz"], st["s2"], st["rot"], st["o2"], st["xi"], 0.05, native=True)
    return dict(xyz=st["xyz"])


def _mcmc_reg(st):
    from diff_gaussian_rasterization import mcmc
    mcmc.add_regularizer_grads(st["o"], st["s"], 0.01, 0.02, st["go"], st["gs"], native=True)
    return dict(go=st["go"], gs=st["gs"])


def _slice_make(seed, device):
    import bilagrid_ref as BR
    grids, image, go = BR.make_inputs(*BR.SHAPES[1], seed=seed)
    return _dev(dict(grids=grids, image=image, go=go), device)


def _slice_run(st):
    import bilagrid_ref as BR
    from diff_gaussian_rasterization.bilagrid import slice_apply
    grids, image = _leaf(st["grids"]), _leaf(st["image"])
    out = slice_apply(grids, image, BR.IDX, native=True)
    dg, di = torch.autograd.grad(out, (grids, image), st["go"])
    return dict(out=out, dgrids=dg, dimage=di)


def _tv_make(shape):
    def make(seed, device):
        import bilagrid_ref as BR
        g = torch.Generator().manual_seed(800 + seed)
        return _dev(dict(grids=BR.make_tv_grids(*shape, seed=seed), up=torch.randn((), generator=g)), device)
    return make


def _tv_run(st):
    from diff_gaussian_rasterization.bilagrid import total_variation_loss
    grids = _leaf(st["grids"])
    tv = total_variation_loss(grids, native=True)
    (dg,) = torch.autograd.grad(tv, grids, st["up"])
    return dict(tv=tv, dgrids=dg)


VQ = (2000, 100, 9)


def _vq_make(seed, device):
    rng = np.random.default_rng(900 + seed)
    P, K, D = VQ
    return _dev(dict(x=rng.standard_normal((P, D)).astype(np.float32), cb=rng.standard_normal((K, D)).astype(np.float32),
                     idx=rng.integers(0, K, P).astype(np.int32)), device)


def _vq_run(st):
    from diff_gaussian_rasterization import vq
    idx, dist2 = vq.assign(st["x"], st["cb"], native=True)
    cb1, counts1 = vq.update_codebook(st["x"], idx, st["cb"], native=True)            # the assignment just computed
    cb2, counts2 = vq.update_codebook(st["x"], st["idx"], st["cb"], native=True)      # a staged one
    return dict(idx=idx, dist2=dist2, cb1=cb1, counts1=counts1, cb2=cb2, counts2=counts2)


F3D_P = 1000


def _f3d_cameras():
    import filter3d_ref as FR
    return FR.posed_trio()[:1]


def _f3d_make(seed, device):
    """filter3d_ref.fixture("posed1", P) with the seed as a parameter: a scene in the posed camera's view space, a tenth behind it."""
    import filter3d_ref as FR
    import posed
    cam = _f3d_cameras()[0]
    xyz = posed.to_world(S.make_scene(F3D_P, 64, 48, 0, 1000 + seed), cam).means3D
    n = F3D_P // 10
    xyz = torch.cat((xyz[:F3D_P - n], FR._behind(cam, n, torch.Generator().manual_seed(1100 + seed))))
    return _dev(dict(xyz=xyz), device)


def _f3d_run(st):
    from diff_gaussian_rasterization.filter3d import compute_filter_3d
    return dict(filter_3D=compute_filter_3d(st["xyz"], _f3d_cameras(), native=True))


def _f3d_apply_make(raw):
    def make(seed, device):
        import filter3d_ref as FR
        (o, s, f), g_o, g_s = FR.apply_case(F3D_P, 1200 + seed, raw)
        return _dev(dict(o=o, s=s, f=f, g_o=g_o, g_s=g_s), device)
    return make


def _f3d_apply_run(raw):
    def run(st):
        from diff_gaussian_rasterization.filter3d import apply_filter_3d
        o, s = _leaf(st["o"]), _leaf(st["s"])
        o2, s2 = apply_filter_3d(o, s, st["f"], raw=raw, native=True)
        d_o, d_s = torch.autograd.grad((o2, s2), (o, s), (st["g_o"], st["g_s"]))
        return dict(o=o2, s=s2, d_o=d_o, d_s=d_s)
    return run


XR_P, XR_FRAC = 4097, 0.5


def _xr_keys():
    """The depth keys of the exchange (as tests/test_gpu_sharded.py draws them) and the key that bounds half of the visible ones: one
    multiset for every seed, which only permutes it, so the host-side row count holds for the decoy too."""
    g = torch.Generator().manual_seed(XR_P)
    vals = torch.randint(0x3E4CCCCD, 0x40C00000, (XR_P,), generator=g, dtype=torch.int64)
    vals[torch.rand(XR_P, generator=g) < 0.25] = 0xFFFFFFFF
    visible = vals[vals != 0xFFFFFFFF].sort().values
    k_max = int(visible[max(int(XR_FRAC * visible.numel()) - 1, 0)])
    return vals.where(vals < 2 ** 31, vals - 2 ** 32).to(torch.int32), k_max, int((visible <= k_max).sum())


def _xr_make(seed, device):
    from diff_gaussian_rasterization import _native as N
    keys, _, _ = _xr_keys()
    g = torch.Generator().manual_seed(1300 + seed)
    desc = N.make_desc(XR_P, 0, 1, 64, 64, 0.5, 0.5, 1.0, False, False)
    geom_ws = torch.zeros(N.workspace_sizes(desc)[0], dtype=torch.uint8, device=device)
    st = _dev(dict(keys=keys[torch.randperm(XR_P, generator=g)], partial=torch.randn(XR_P, 12, generator=g),
                   screen=torch.randn(XR_P, 12, generator=g)), device)
    return dict(st, geom_ws=geom_ws, desc=desc)


def _xr_staged(st):
    return [st["keys"], st["partial"], st["screen"]]


def _xr_run(st):
    from diff_gaussian_rasterization import _native as N
    _, k_max, n = _xr_keys()
    N.frame_arrays(st["desc"], st["geom_ws"])[0].copy_(st["keys"])                   # (torch, on the current stream)
    rows, packed = N.exchange_rows_gather(st["desc"], st["geom_ws"], k_max, st["partial"], n)
    N.exchange_rows_scatter(st["desc"], rows, packed, st["screen"])
    return dict(rows=rows, packed=packed, screen=st["screen"])


SORT_N = 5000


def _sort_make(seed, device):
    g = torch.Generator().manual_seed(1700 + seed)
    return _dev(dict(keys=torch.randint(-2 ** 31, 2 ** 31 - 1, (SORT_N,), generator=g, dtype=torch.int64).to(torch.int32),
                     vals=torch.randperm(SORT_N, generator=g).to(torch.int32)), device)


def _sort_run(st):
    """The library's radix sort with its count on the device: the call uploads the count and waits for the stream."""
    from diff_gaussian_rasterization import _native as N
    k, v = N.debug_sort_pairs(st["keys"], st["vals"], 32, count_on_device=True)
    return dict(keys=k, vals=v)


LOSS_SHAPE = (3, 67, 96)


def _loss_make(seed, device):
    import loss_ref as LR
    a, b = LR.smooth_pair(*LOSS_SHAPE, 0.05, seed=1400 + seed)
    return _dev(dict(a=a, b=b, up=torch.rand((), generator=torch.Generator().manual_seed(seed)) + 0.5), device)


def _loss_fused(st):
    from loss_utils import training_loss
    a = _leaf(st["a"])
    loss = training_loss(a, st["b"], 0.2)
    return dict(loss=loss, grad=torch.autograd.grad(loss, a, st["up"])[0])


def _loss_pair(st):
    from loss_utils import l1_loss, ssim
    a = _leaf(st["a"])
    Ll1 = l1_loss(a, st["b"])
    sim = ssim(a, st["b"])                              # shares the first call's fused forward
    loss = (1.0 - 0.2) * Ll1 + 0.2 * (1.0 - sim)
    return dict(l1=Ll1, ssim=sim, loss=loss, grad=torch.autograd.grad(loss, a, st["up"])[0])


def _loss_rows(st):
    from loss_utils import training_loss_rows
    a = _leaf(st["a"])
    loss = training_loss_rows(a, st["b"], 0.2, (16, 48), lambda t: t)
    return dict(loss=loss, grad=torch.autograd.grad(loss, a, st["up"])[0])


# ---- the rasterizer -------------------------------------------------------------------------------------------------------------------

GEOM = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")
CAM = ("viewmatrix", "projmatrix", "campos")


def _frame_make(P, W, H, D, scale=(0.005, 0.06), precomp=False, upper_half=False, seed_of=lambda s: s):
    def make(seed, device):
        seed = seed_of(seed)
        scene = S.make_scene(P, W, H, D, seed, scale_lo=scale[0], scale_hi=scale[1])
        if upper_half:                      # (tests/test_gpu_parity.py::test_binning_workspace_is_capped_and_grows_on_demand)
            scene.means3D[:, 1] = -scene.means3D[:, 1].abs() - 0.02 * scene.means3D[:, 2]
        extra = {}
        if precomp:
            a = scene.activated()
            extra = dict(colors_precomp=torch.rand(P, 3, generator=torch.Generator().manual_seed(seed)),
                         cov3D_precomp=cov3d_from(a["scales"], a["rotations"]))
        kw = raster_kwargs(scene, S.make_camera(W, H), bg=(0.1, 0.2, 0.3), as_numpy=False, **extra)
        g = torch.Generator().manual_seed(seed + 1)
        st = {k: kw[k] for k in GEOM + CAM + ("bg",) if kw.get(k) is not None}
        st.update(gimg=S.make_grad_image(W, H, seed), gdepth=torch.rand(1, H, W, generator=g) - 0.5, galpha=torch.rand(1, H, W, generator=g) - 0.5,
                  target=torch.rand(3, H, W, generator=g))
        st = _dev({k: v.float() for k, v in st.items()}, device)
        st["meta"] = dict(P=P, W=W, H=H, D=D, tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"])
        return st
    return make


def _frame_forward(st, depth_alpha=False, antialiasing=False, absgrad=False, cam_grad=False, debug=False):
    """The standard API's forward on leaves over the staged buffers -> (outputs, leaves by name)."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    m = st["meta"]
    leaves = {k: _leaf(st[k]) for k in GEOM if k in st}
    cam = {k: (_leaf(st[k]) if cam_grad else st[k]) for k in CAM}
    rs = GaussianRasterizationSettings(m["H"], m["W"], m["tanfovx"], m["tanfovy"], st["bg"], 1.0, cam["viewmatrix"], cam["projmatrix"], m["D"],
                                       cam["campos"], False, debug)
    means2D = torch.zeros(m["P"], 3, device=st["bg"].device, requires_grad=True)
    out = GaussianRasterizer(rs, depth_alpha=depth_alpha, antialiasing=antialiasing, absgrad=absgrad)(means2D=means2D, **leaves)
    leaves["means2D"] = means2D
    if cam_grad:
        leaves.update(cam)
    return out, leaves


def _frame_run(**flags):
    def run(st):
        out, leaves = _frame_forward(st, **flags)
        res = dict(color=out[0], radii=out[1])
        outs, ups = [out[0]], [st["gimg"]]
        if flags.get("depth_alpha"):
            res.update(depth=out[2], alpha=out[3])
            outs, ups = outs + [out[2], out[3]], ups + [st["gdepth"], st["galpha"]]
        ST.between(*ups)
        grads = torch.autograd.grad(outs, list(leaves.values()), ups)
        res.update({"d_" + k: g for k, g in zip(leaves, grads)})
        if flags.get("absgrad"):
            res["absgrad"] = leaves["means2D"].absgrad
        return res
    return run


def _mark_visible_run(st):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    m = st["meta"]
    rs = GaussianRasterizationSettings(m["H"], m["W"], m["tanfovx"], m["tanfovy"], st["bg"], 1.0, st["viewmatrix"], st["projmatrix"], m["D"],
                                       st["campos"], False, False)
    return dict(visible=GaussianRasterizer(rs).markVisible(st["means3D"]))


def _frame_staged(st):
    return [v for k, v in st.items() if k != "meta"]


def _growth_run(st):
    """The frame with no workspace guess: the first attempt of stage 2 ends with ERR_WORKSPACE and the frame is re-run with room for R."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    dgr._binning_guess.clear()
    errors, orig = [], N.forward_render

    def spy(*a, **k):
        try:
            return orig(*a, **k)
        except N.GsrError as e:
            errors.append(e.status)
            raise
    N.forward_render = spy
    try:
        res = _frame_run()(st)
    finally:
        N.forward_render = orig
        dgr._binning_guess.clear()
    assert errors == [N.ERR_WORKSPACE], errors
    return res


def _model_make(kind, P=6000, W=200, H=136, D=2):
    def make(seed, device):
        from gaussian_params import GaussianParams, Pipe
        scene = S.make_scene(P, W, H, D, 1500 + seed, scale_lo=0.005, scale_hi=0.06)
        pipe = Pipe()
        if kind == "model":
            from scene import GaussianModel
            from scene.gaussian_model import TABLE
            pc = GaussianModel(D)
            pc.adopt_scene(scene, device=device)
            params = [pc._t[k] for k in TABLE]
        else:
            pc = GaussianParams(scene).to(device)
            pipe.fused_activations = True
            params = list(pc.parameters())
        return dict(pc=pc, pipe=pipe, params=params, cam=S.make_camera(W, H).to(device), bg=torch.tensor([0.1, 0.2, 0.3], device=device),
                    gimg=S.make_grad_image(W, H, seed).to(device),
                    target=torch.rand(3, H, W, generator=torch.Generator().manual_seed(1600 + seed)).to(device))
    return make


def _model_staged(st):
    return st["params"] + [st["gimg"], st["target"]]


def _model_run(st):
    from gaussian_renderer import render
    out = render(st["cam"], st["pc"], st["pipe"], st["bg"])
    ST.between(st["gimg"])
    grads = torch.autograd.grad(out["render"], st["params"] + [out["viewspace_points"]], st["gimg"])
    return dict(render=out["render"], radii=out["radii"], **{f"d{i}": g for i, g in enumerate(grads)})


FRAME_A = dict(P=5000, W=256, H=192, D=3)
FRAME_B = dict(P=2048, W=128, H=128, D=3)
_seed_a = lambda s: {1: 109, 2: 110}[s]
_seed_b = lambda s: {1: 105, 2: 106}[s]


def _frame_case(name, make, run=None, **flags):
    return ST.Case(name, make, _frame_staged, run or _frame_run(**flags), blocking=True)


def _dict_case(name, make, run, blocking=False):
    return ST.Case(name, make, _all, run, blocking=blocking)


ELEMENTWISE = [
    _dict_case("activations", _act_make, _act_run),
    ST.Case("fused_adam", _adam_make(False), _adam_staged, _adam_run),
    ST.Case("sparse_fused_adam", _adam_make(True), _adam_staged, _adam_run),
    _dict_case("densify_stats", _densify_make, _densify_run),
    _dict_case("distCUDA2", _knn_make, _knn_run),
    _dict_case("compose_structures", _compose_make, _compose_run),
    _dict_case("decoder_B1", _decoder_make((1, 32, False, 1, 1)), _decoder_run),
    _dict_case("decoder_B257_embedding", _decoder_make((257, 32, True, 8, 16)), _decoder_run),
    _dict_case("mcmc_relocation", _mcmc_make, _mcmc_relocation),
    _dict_case("mcmc_relocate_rows", _mcmc_make, _mcmc_rows),
    _dict_case("mcmc_noise", _mcmc_make, _mcmc_noise),
    _dict_case("mcmc_reg_grads", _mcmc_make, _mcmc_reg),
    _dict_case("bilagrid_slice_apply", _slice_make, _slice_run),
    _dict_case("bilagrid_tv_1x1x1x1", _tv_make((1, 1, 1, 1)), _tv_run),
    _dict_case("bilagrid_tv_2x2x3x4", _tv_make((2, 2, 3, 4)), _tv_run),
    _dict_case("vq_assign_update", _vq_make, _vq_run),
    _dict_case("filter3d_compute", _f3d_make, _f3d_run, blocking=True),
    _dict_case("filter3d_apply", _f3d_apply_make(False), _f3d_apply_run(False)),
    _dict_case("filter3d_apply_raw", _f3d_apply_make(True), _f3d_apply_run(True)),
    ST.Case("exchange_rows", _xr_make, _xr_staged, _xr_run),
    _dict_case("radix_sort_count_on_device", _sort_make, _sort_run, blocking=True),
    _dict_case("training_loss", _loss_make, _loss_fused),
    _dict_case("l1_loss_then_ssim", _loss_make, _loss_pair),
    _dict_case("training_loss_rows", _loss_make, _loss_rows),
]
_frame_a = _frame_make(**FRAME_A, seed_of=_seed_a)
FRAMES = [
    ST.Case("mark_visible", _frame_a, _frame_staged, _mark_visible_run),
    _frame_case("frame", _frame_a),
    _frame_case("frame_depth_alpha", _frame_a, depth_alpha=True),
    _frame_case("frame_antialiasing", _frame_a, antialiasing=True),
    _frame_case("frame_absgrad", _frame_a, absgrad=True),
    _frame_case("frame_camera_grads", _frame_a, cam_grad=True),
    _frame_case("frame_debug", _frame_a, debug=True),
    _frame_case("frame_precomp", _frame_make(2048, 128, 128, 3, precomp=True, seed_of=_seed_b)),
    ST.Case("render_gaussian_model", _model_make("model"), _model_staged, _model_run, blocking=True),
    ST.Case("render_params_fused_activations", _model_make("params"), _model_staged, _model_run, blocking=True),
    _frame_case("frame_depth_chunks", _frame_make(60_000, 320, 200, 1, scale=(0.02, 0.2), seed_of=lambda s: 4 + s)),
    _frame_case("frame_workspace_growth", _frame_make(150_000, 640, 368, 1, scale=(0.01, 0.08), upper_half=True, seed_of=lambda s: 76 + s),
                run=_growth_run),
]
_BY_NAME = {c.name: c for c in ELEMENTWISE + FRAMES}


@pytest.fixture(scope="module")
def delay():
    """The references of every op (with them the host time of every enqueue that does not wait for the device: the non-blocking ops
    whole, the frames' backward), then the delay: >= 20 ms and >= 10 x the slowest."""
    for case in ELEMENTWISE + FRAMES:
        ST.default_run(case, DEV)
    d = ST.Delay.on(DEV)
    slowest = max(ST.HOST_MS, key=ST.HOST_MS.get)
    d.set(max(ST.DELAY_MS, 10.0 * ST.HOST_MS[slowest]))
    print(f"\nMEASURED delay {d.ms:.1f} ms ({d.count} matmuls of {d.n}^2, {d.per_ms:.3f} ms each); slowest non-blocking enqueue: "
          f"{slowest} {ST.HOST_MS[slowest]:.3f} ms; all: " + ", ".join(f"{k} {v:.2f}" for k, v in ST.HOST_MS.items()))
    assert d.ms >= ST.DELAY_MS and d.ms >= 10.0 * max(ST.HOST_MS.values())
    return d


@pytest.mark.parametrize("case", ELEMENTWISE + FRAMES, ids=repr)
def test_side_stream_run_equals_the_default_stream_run(case, side, delay):
    ST.check_on_side_stream(case, side, DEV)


# ---- the harness detects what it is for ------------------------------------------------------------------------------------------------

ACT_FWD = _dict_case("activations_forward", _act_make, _act_fwd)
ADAM_DENSE = ST.Case("fused_adam_step", _adam_make(False), _adam_staged, _adam_run)


def _snapshot_on(stream):
    """Adam steps in place and the staged copy of the real inputs lands on the same buffers later: what the step computed is read
    behind it on the stream it was (wrongly) given."""
    def after(st):
        with torch.cuda.stream(stream):
            return {k: v.clone() for k, v in _adam_result(st).items()}
    return after


@pytest.mark.parametrize("variant", ("second_stream", "null_stream"))
def test_sensitivity_a_wrong_stream_computes_the_decoy(variant, N, side, delay, monkeypatch):
    """_native._stream patched for the duration of the call: (a) a second torch stream, (b) the null stream.  Both ops take every
    address and loop bound from host-side sizes, so running them on the decoy is a valid computation.  Either way the op runs while
    `side` is still in its delay: the result is the default-stream result of the DECOY, bit for bit."""
    other = torch.cuda.Stream(device=DEV) if variant == "second_stream" else torch.cuda.default_stream(DEV)
    handle = other.cuda_stream if variant == "second_stream" else 0
    monkeypatch.setattr(N, "_stream", lambda device: ctypes.c_void_p(handle))
    try:
        got = ST.side_run(ACT_FWD, side, DEV)
        adam, snap = ST.side_run(ADAM_DENSE, side, DEV, after=_snapshot_on(other))
        torch.cuda.synchronize()
        snap = ST.cpu_bits(snap)
    finally:
        monkeypatch.undo()
        torch.cuda.synchronize()                       # before any buffer of these runs goes out of scope
    want_real, want_decoy = ST.default_run(ACT_FWD, DEV), ST.default_run(ACT_FWD, DEV, seed=ACT_FWD.decoy)
    assert set(ST.differ(want_real, want_decoy)) == set(want_real)
    ST.assert_same(got, want_decoy, f"activations forward on the {variant}")
    adam_decoy = ST.default_run(ADAM_DENSE, DEV, seed=ADAM_DENSE.decoy)
    ST.assert_same(snap, adam_decoy, f"the Adam step on the {variant}")
    # ... and the staged copy then overwrote it: the buffers hold the real inputs, not stepped at all
    st = ADAM_DENSE.make(ADAM_DENSE.seed, DEV)
    ST.assert_same(adam, ST.cpu_bits(_adam_result(st)), "the buffers after the staged copy")


def test_harness_passes_with_the_right_stream_and_fails_on_a_different_result(side, delay):
    """The same two ops, unpatched, pass; and real and decoy differ in every output (a comparison that could not fail proves nothing)."""
    for case in (ACT_FWD, ADAM_DENSE):
        ST.check_on_side_stream(case, side, DEV)
        real, decoy = ST.default_run(case, DEV), ST.default_run(case, DEV, seed=case.decoy)
        assert set(ST.differ(decoy, real)) == set(real), case


# ---- profiling, two streams, a thread, a second device -----------------------------------------------------------------------------------

def test_profile_counts_on_a_side_stream_equal_the_default_stream(N, side, delay):
    case = _BY_NAME["frame"]

    def counted(run):
        N.profile_enable(True)
        try:
            got = run()
            torch.cuda.synchronize()
            return got, {k: v[1] for k, v in N.profile_read(64).items()}
        finally:
            N.profile_enable(False)
    ST.default_run(case, DEV)                                        # (the workspace guess of this frame shape is warm either way)
    want, counts_default = counted(lambda: ST.default_run(case, DEV, cache=False))
    got, counts_side = counted(lambda: ST.side_run(case, side, DEV))
    ST.assert_same(got, want, "profiled frame")
    assert counts_default and len(counts_default) >= 5, counts_default
    # default_run runs the frame twice, the side run once
    assert {k: 2 * v for k, v in counts_side.items()} == counts_default, (counts_side, counts_default)


class _Steps:
    """A frame and its loss in the pieces the two-stream test interleaves.  kind "rasterizer": the standard API and training_loss();
    kind "render": render() on a parameter store (the shared block of zeros behind viewspace_points), then l1_loss() and ssim() as
    train.py composes them (the second call looks for the first one's fused forward in loss_utils._shared)."""

    def __init__(self, st, kind):
        self.st, self.kind = st, kind

    def forward(self):
        if self.kind == "rasterizer":
            out, leaves = _frame_forward(self.st)
            self.image, self.radii, self.names, self.wrt = out[0], out[1], list(leaves), list(leaves.values())
        else:
            from gaussian_renderer import render
            out = render(self.st["cam"], self.st["pc"], self.st["pipe"], self.st["bg"])
            self.image, self.radii = out["render"], out["radii"]
            self.wrt = self.st["params"] + [out["viewspace_points"]]
            self.names = [str(i) for i in range(len(self.wrt))]

    def loss(self):
        from loss_utils import training_loss
        self.value = training_loss(self.image, self.st["target"], 0.2)

    def l1(self):
        from loss_utils import l1_loss
        self.l1_value = l1_loss(self.image, self.st["target"])

    def ssim(self):
        from loss_utils import ssim
        self.value = (1.0 - 0.2) * self.l1_value + 0.2 * (1.0 - ssim(self.image, self.st["target"]))

    def backward(self):
        self.grads = torch.autograd.grad(self.value, self.wrt)

    def result(self):
        return dict(image=self.image, radii=self.radii, loss=self.value, **{"d_" + k: g for k, g in zip(self.names, self.grads)})


def _steps_run(kind):
    def run(st):
        f = _Steps(st, kind)
        f.forward()
        if kind == "rasterizer":
            f.loss()
        else:
            f.l1(); f.ssim()
        ST.between()
        f.backward()
        return f.result()
    return run


IN_FLIGHT = {
    "rasterizer": (ST.Case("frame_A_with_loss", _frame_a, _frame_staged, _steps_run("rasterizer"), blocking=True),
                   ST.Case("frame_B_with_loss", _frame_make(**FRAME_B, seed_of=_seed_b), _frame_staged, _steps_run("rasterizer"), blocking=True)),
    "render": (ST.Case("render_A_with_l1_ssim", _model_make("model"), _model_staged, _steps_run("render"), blocking=True),
               ST.Case("render_B_with_l1_ssim", _model_make("params", P=3000, W=160, H=112), _model_staged, _steps_run("render"), blocking=True)),
}


@pytest.mark.parametrize("kind", sorted(IN_FLIGHT))
def test_two_frames_in_flight_on_two_streams(kind, delay):
    """Forward A on s1, forward B on s2, the loss on each, backward B, backward A, from one host thread, each stream behind its own
    delay: every output and gradient equals the frame run alone.  "rasterizer": the standard API and training_loss (the readback
    sequence of the thread, _binning_guess).  "render": two parameter stores of different sizes through render() (_ZERO_POINTS is
    re-made under a frame in flight) and l1_loss(A), l1_loss(B), ssim(A), ssim(B): B's fused forward replaces A's in
    loss_utils._shared before A's ssim asks for it, which then computes its own."""
    case_a, case_b = IN_FLIGHT[kind]
    want = {c.name: ST.default_run(c, DEV) for c in (case_a, case_b)}
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    work = {c.name: c.make(c.decoy, DEV) for c in (case_a, case_b)}
    real = {c.name: c.make(c.seed, DEV) for c in (case_a, case_b)}
    torch.cuda.synchronize()
    a, b = _Steps(work[case_a.name], kind), _Steps(work[case_b.name], kind)
    for s, c in ((s1, case_a), (s2, case_b)):
        with torch.cuda.stream(s):
            delay()
            ST.stage(work[c.name], real[c.name], c)
    losses = ((s1, a.loss), (s2, b.loss)) if kind == "rasterizer" else ((s1, a.l1), (s2, b.l1), (s1, a.ssim), (s2, b.ssim))
    for s, step in ((s1, a.forward), (s2, b.forward)) + losses + ((s2, b.backward), (s1, a.backward)):
        with torch.cuda.stream(s):
            step()
    s1.synchronize(); s2.synchronize()
    got = {case_a.name: ST.cpu_bits(a.result()), case_b.name: ST.cpu_bits(b.result())}
    torch.cuda.synchronize()
    for name in want:
        ST.assert_same(got[name], want[name], f"{name}, two frames in flight")


def test_total_variation_alternating_on_two_streams(delay):
    """Three calls on each of two streams, alternating, different grids every time: the per-(device, stream) ticket workspace."""
    cases = [ST.Case(f"tv_{i}", _tv_make(shape), _all, _tv_run, seed=10 + i, decoy=20 + i)
             for i, shape in enumerate(((3, 8, 16, 16), (2, 2, 3, 4), (3, 8, 16, 16), (1, 1, 1, 1), (2, 2, 3, 4), (3, 8, 16, 16)))]
    want = [ST.default_run(c, DEV) for c in cases]
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    work, real = [c.make(c.decoy, DEV) for c in cases], [c.make(c.seed, DEV) for c in cases]
    torch.cuda.synchronize()
    for k, s in enumerate(streams):
        with torch.cuda.stream(s):
            delay()
            for i in range(k, len(cases), 2):
                ST.stage(work[i], real[i], cases[i])
    outs = []
    for i, c in enumerate(cases):                                   # case i on stream i % 2
        with torch.cuda.stream(streams[i % 2]):
            outs.append(c.run(work[i]))
    for s in streams:
        s.synchronize()
    got = [ST.cpu_bits(o) for o in outs]
    torch.cuda.synchronize()
    for c, g, w in zip(cases, got, want):
        ST.assert_same(g, w, f"{c.name} alternating on two streams")


def test_frame_from_a_fresh_host_thread(delay):
    """Forward and backward issued from a new thread (its own control-block readback) on a side stream of its own."""
    case = _BY_NAME["frame"]
    want = ST.default_run(case, DEV)
    box = {}

    def work():
        try:
            box["got"] = ST.side_run(case, torch.cuda.Stream(device=DEV), DEV)
        except BaseException as e:                 # reported by the main thread
            box["error"] = e
    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(timeout=120.0)
    assert not t.is_alive(), "the frame issued from a fresh thread did not finish within 120 s"
    if "error" in box:
        raise box["error"]
    ST.assert_same(box["got"], want, "frame from a fresh host thread")


SECOND_DEVICE = ("frame", "training_loss", "fused_adam", "bilagrid_tv_2x2x3x4", "vq_assign_update", "filter3d_compute")


@pytest.mark.parametrize("name", SECOND_DEVICE)
def test_second_device(name):
    """Inputs on cuda:1 while the current device stays cuda:0: outputs on cuda:1, bit-equal to the cuda:0 run; the same on a side stream
    of cuda:1.  One process, no children."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"needs two devices, this machine shows {n}")
    case, dev1 = _BY_NAME[name], "cuda:1"
    want = ST.default_run(case, DEV)
    torch.cuda.set_device(0)
    state = case.make(case.seed, dev1)
    torch.cuda.synchronize(dev1)
    outs = case.run(state)
    assert torch.cuda.current_device() == 0
    assert all(v.device == torch.device(dev1) for v in outs.values() if v is not None), {k: v.device for k, v in outs.items()}
    torch.cuda.synchronize(dev1)
    ST.assert_same(ST.cpu_bits(outs), want, f"{name} on {dev1}, current device cuda:0")
    got = ST.side_run(case, torch.cuda.Stream(device=dev1), dev1, enter=False)
    assert torch.cuda.current_device() == 0
    ST.assert_same(got, want, f"{name} on a side stream of {dev1}")
