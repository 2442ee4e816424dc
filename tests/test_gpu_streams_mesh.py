"""Mesh cleaning on a side stream and on two streams (tests/streams.py's protocol, as tests/test_gpu_streams.py runs it for every other
op): face_components and clean_mesh, issued on a side stream behind a delay while the faces are still the decoy's, give the integers
of the default-stream run.  A launch, memset or copy of the feature on any other stream - the union-find's start, the link and label
passes, the threshold's topk, the used flags' clear, the scan, the two emit passes, the gathers - would run early, on the decoy or on a
workspace nothing has written yet, and show.  The decoy is another shuffle of the same mesh: valid indices, the same shapes."""
import pytest
import torch

import mesh_ref as MR
import streams as ST

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _make(seed, device):
    V, f = MR.islands(seed=100 + seed)
    g = torch.Generator().manual_seed(300 + seed)
    return dict(faces=torch.as_tensor(f).to(device).contiguous(), vertices=torch.randn(V, 3, generator=g).to(device),
                colors=torch.rand(V, 3, generator=g).to(device))


def _staged(st):
    return [st["faces"], st["vertices"], st["colors"]]


def _components_run(st):
    from diff_gaussian_rasterization.meshops import face_components
    labels, sizes = face_components(st["faces"], st["vertices"].shape[0], native=True)
    return dict(labels=labels, sizes=sizes)


def _clean_run(kw):
    def run(st):
        from diff_gaussian_rasterization.meshops import clean_mesh
        v, f, c, vsrc, fsrc = clean_mesh(st["vertices"], st["faces"], st["colors"], return_index=True, native=True, **kw)
        return dict(vertices=v, faces=f, colors=c, vertex_src=vsrc, face_src=fsrc)
    return run


COMPONENTS = ST.Case("mesh_face_components", _make, _staged, _components_run)
CLEAN = ST.Case("mesh_clean_min_faces", _make, _staged, _clean_run(dict(min_faces=2)), blocking=True)
CLEAN_LARGEST = ST.Case("mesh_clean_keep_largest", _make, _staged, _clean_run(dict(keep_largest=1)), blocking=True, seed=3, decoy=4)


@pytest.fixture(scope="module")
def delay():
    """The references first (with them the host time of the one enqueue that does not wait for the device), then the delay: at least
    20 ms and at least 10 x that time."""
    for case in (COMPONENTS, CLEAN, CLEAN_LARGEST):
        ST.default_run(case, DEV)
    d = ST.Delay.on(DEV)
    d.set(max(ST.DELAY_MS, 10.0 * ST.HOST_MS[COMPONENTS.name]))
    assert d.ms >= 10.0 * ST.HOST_MS[COMPONENTS.name]
    return d


@pytest.mark.parametrize("case", [COMPONENTS, CLEAN, CLEAN_LARGEST], ids=repr)
def test_mesh_cleaning_on_a_side_stream(case, delay):
    want = ST.default_run(case, DEV)
    decoy = ST.default_run(case, DEV, seed=case.decoy)
    assert ST.differ(decoy, want), "the decoy gives the real result: the comparison could not fail"
    if case is not COMPONENTS:
        assert want["faces"].shape == (300, 3) and want["vertex_src"].shape == (176,)
    ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)


def test_mesh_cleaning_alternating_on_two_streams(delay):
    """Components and cleanings of different meshes on two streams, alternating from one host thread, each stream behind its own delay:
    every call has a workspace of its own, so each result equals the call run alone."""
    kinds = (COMPONENTS, CLEAN, CLEAN_LARGEST, COMPONENTS, CLEAN, CLEAN_LARGEST)
    cases = [ST.Case(f"{k.name}_{i}", k.make, k.staged, k.run, seed=10 + i, decoy=20 + i, blocking=k.blocking) for i, k in enumerate(kinds)]
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
