"""A camera with a small differentiable rigid correction: the only pose code of the package.

The rasterizer returns dL/dviewmatrix, dL/dprojmatrix and dL/dcampos separately, one per tensor as its forward consumed it
(diff_gaussian_rasterization, "Camera gradients"); a caller chains them to whatever pose parametrisation it uses through its own
torch graph.  camera_with_pose_delta is the smallest such graph: six numbers, enough for refining approximately known poses and
for tracking a camera against a fixed model.
"""
import copy
import math

import torch


def _projection(cam, dtype, device) -> torch.Tensor:
    """The camera's projection matrix in the row-vector convention (scene_synth.projection_matrix, transposed)."""
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    zn, zf = float(cam.znear), float(cam.zfar)
    Pm = torch.zeros(4, 4, dtype=dtype, device=device)
    Pm[0, 0], Pm[1, 1] = 1.0 / tx, 1.0 / ty
    Pm[2, 2], Pm[2, 3] = zf / (zf - zn), 1.0
    Pm[3, 2] = -(zf * zn) / (zf - zn)
    return Pm


def camera_with_pose_delta(cam, rot_vec: torch.Tensor, trans: torch.Tensor):
    """A copy of `cam` whose world_view_transform, full_proj_transform and camera_center are differentiable torch functions of a
    rigid correction applied in the camera's own frame: p_view' = exp(hat(rot_vec)) p_view + trans.  In the row-vector convention
    of the matrices (p_view = [p, 1] @ V):   V' = V @ E,  E = [[exp(hat(rot_vec))^T, 0], [trans, 1]];   PV' = V' @ P;
    centre = -t' R'^T with V' = [[R', 0], [t', 1]].  At rot_vec = trans = 0 the three equal the camera's own (to rounding: the
    projection is rebuilt from FoVx / FoVy).  Computed in rot_vec's dtype."""
    dtype, device = rot_vec.dtype, cam.world_view_transform.device
    V = cam.world_view_transform.to(dtype)
    zero = torch.zeros((), dtype=dtype, device=device)
    rx, ry, rz = rot_vec.to(device).unbind(0)
    hat = torch.stack([torch.stack([zero, -rz, ry]), torch.stack([rz, zero, -rx]), torch.stack([-ry, rx, zero])])
    Rd = torch.linalg.matrix_exp(hat)
    E = torch.zeros(4, 4, dtype=dtype, device=device)
    E[3, 3] = 1.0
    E = E + torch.nn.functional.pad(Rd.t(), (0, 1, 0, 1)) + torch.nn.functional.pad(trans.to(device).view(1, 3), (0, 1, 3, 0))
    Vn = V @ E
    out = copy.copy(cam)
    out.world_view_transform = Vn
    out.full_proj_transform = Vn @ _projection(cam, dtype, device)
    out.camera_center = -(Vn[3, :3] @ Vn[:3, :3].t())
    return out
