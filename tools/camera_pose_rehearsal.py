"""CPU rehearsal of tests/test_gpu_camera_grad.py::test_pose_recovery at reduced size: the same loop (camera_with_pose_delta,
Adam on the training loss, the same start offset, learning rate and step count) with the binary64 reference renderer
tests/torch_ref.render_autograd in place of the rasterizer.  Prints the loss and the pose errors; the reference must meet the test's
conditions with room before the learning rate and the step count go into the test.

    python tools/camera_pose_rehearsal.py [--P 300] [--lr 1e-3] [--steps 150]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    from camera_ref import POSE_LR, POSE_START, POSE_STEPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=300)
    ap.add_argument("--lr", type=float, default=POSE_LR)
    ap.add_argument("--steps", type=int, default=POSE_STEPS)
    a = ap.parse_args()
    import posed as PO
    import scene_synth as S
    from loss_utils import training_loss_torch
    from scene.cameras import camera_with_pose_delta
    from torch_ref import render_autograd
    W, H = 64, 48
    cam = PO.posed_camera(W, H, "a")
    scene = PO.to_world(S.make_scene(a.P, W, H, 3, 11, scale_lo=0.02, scale_hi=0.2, zmin=1.0), cam)
    act = {k: v.double() for k, v in scene.activated().items()}

    def image(c):
        return render_autograd(image_height=H, image_width=W, tanfovx=math.tan(c.FoVx * 0.5), tanfovy=math.tan(c.FoVy * 0.5),
                               bg=torch.zeros(3, dtype=torch.float64), scale_modifier=1.0, viewmatrix=c.world_view_transform,
                               projmatrix=c.full_proj_transform, sh_degree=3, campos=c.camera_center, **act)[0]
    zero = torch.zeros(3, dtype=torch.float64)
    with torch.no_grad():
        target = image(camera_with_pose_delta(cam, zero, zero))
    rot = torch.tensor(POSE_START["rot"], dtype=torch.float64, requires_grad=True)
    trans = torch.tensor(POSE_START["trans"], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([rot, trans], lr=a.lr)
    r0, t0 = float(rot.detach().norm()), float(trans.detach().norm())
    for step in range(a.steps):
        opt.zero_grad()
        loss = training_loss_torch(image(camera_with_pose_delta(cam, rot, trans)), target)
        loss.backward()
        opt.step()
        if step % 10 == 0 or step == a.steps - 1:
            print(f"step {step:4d} loss {float(loss):.6f} rotation error {math.degrees(float(rot.detach().norm())):.4f} deg "
                  f"(start {math.degrees(r0):.4f}) translation error {float(trans.detach().norm()):.5f} (start {t0:.5f})", flush=True)


if __name__ == "__main__":
    main()
