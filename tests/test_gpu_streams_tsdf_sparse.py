"""The sparse TSDF volume on a side stream and on two streams (tests/streams.py's protocol, as tests/test_gpu_streams_mesh.py runs it for
mesh cleaning): allocate, commit, integrate and extract_mesh, issued on a side stream behind a delay while the maps are still the
decoy's, give the bits of the default-stream run.  A launch, fill or copy of the feature on any other stream - the volume's own
buffers, the marks, the commit's count, scan and assignment, the pool's growth, the fusion, the three extraction stages - would run
early, on the decoy or on a workspace nothing has written yet, and show.  The decoy is another draw of the same frames' noise and
holes: valid maps, the same shapes."""
import pytest
import torch

import streams as ST
import tsdf_ref as TR
from test_tsdf_sparse_ref import TWIN_GRID, sparse_volume

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _make(seed, device):
    frames = TR.make_frames(48, 40, seed=seed)
    st = {}
    for i, fr in enumerate(frames):
        st.update({f"depth{i}": fr.depth[None], f"alpha{i}": fr.alpha[None], f"color{i}": fr.color, f"V{i}": fr.V})
    out = {k: torch.as_tensor(v).to(device).contiguous() for k, v in st.items()}
    out["frames"] = frames
    return out


def _staged(st):
    return [v for v in st.values() if isinstance(v, torch.Tensor)]


def _run(two_pass):
    def run(st):
        vol = sparse_volume(TWIN_GRID, st["depth0"].device, capacity=8)                  # a small pool: it grows on the way
        frames = st["frames"]
        kw = lambda fr: dict(alpha_min=fr.alpha_min, depth_max=fr.depth_max, native=True)
        for step in (("allocate", "integrate") if two_pass else ("both",)):
            for i, fr in enumerate(frames):
                if step != "integrate":
                    vol.allocate(st[f"depth{i}"], st[f"alpha{i}"], st[f"V{i}"], fr.tanfovx, fr.tanfovy, **kw(fr))
                if step != "allocate":
                    vol.integrate(st[f"depth{i}"], st[f"alpha{i}"], st[f"color{i}"], st[f"V{i}"], fr.tanfovx, fr.tanfovy, **kw(fr))
        v, f, c, cells = vol.extract_mesh(return_cells=True, native=True)
        return dict(table=vol.brick_table, coords=vol.brick_coords, tsdf=vol.tsdf, weight=vol.weight, color=vol.color, vertices=v, faces=f,
                    colors=c, cells=cells)
    return run


TWO_PASS = ST.Case("tsdf_sparse_two_pass", _make, _staged, _run(True), blocking=True)
STREAMING = ST.Case("tsdf_sparse_streaming", _make, _staged, _run(False), blocking=True, seed=3, decoy=4)


@pytest.mark.parametrize("case", [TWO_PASS, STREAMING], ids=repr)
def test_the_sparse_volume_on_a_side_stream(case):
    want = ST.default_run(case, DEV)
    decoy = ST.default_run(case, DEV, seed=case.decoy)
    assert ST.differ(decoy, want), "the decoy gives the real result: the comparison could not fail"
    assert want["faces"].shape[0] > 0 and want["table"].shape == (5, 5, 5) and want["tsdf"].shape[0] == want["coords"].shape[0] > 8
    ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)


def test_sparse_volumes_alternating_on_two_streams():
    """Volumes of different frames on two streams, alternating from one host thread, each stream behind its own delay: every volume
    has buffers and workspaces of its own, so each result equals the call run alone."""
    kinds = (TWO_PASS, STREAMING, TWO_PASS, STREAMING)
    cases = [ST.Case(f"{k.name}_{i}", k.make, k.staged, k.run, seed=10 + i, decoy=20 + i, blocking=True) for i, k in enumerate(kinds)]
    want = [ST.default_run(c, DEV) for c in cases]
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    delay = ST.Delay.on(DEV)
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
