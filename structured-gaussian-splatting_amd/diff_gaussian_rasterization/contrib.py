"""Per-Gaussian blend statistics: what every Gaussian contributes to the views it is rendered into (LightGaussian's global
significance, RadSplat's maximum blend weight, Mini-Splatting's and Taming-3DGS's importance scores all start from these).

A pixel composites a splat when the blend gives it a weight w = alpha T > 0 - the event that advances the pixel's contributor
count.  A ContributionStats holds, per Gaussian and over every pixel of every frame rendered into it,

    count           int64   [P]   the pixels that composited it
    weight_sum_q32  int64   [P]   the sum of its w, in units of 2^-32 (weight_sum: the same as float64)
    weight_max      float32 [P]   its largest single w

Pass one to GaussianRasterizer(settings, contributions=stats) (or gaussian_renderer.render(..., contributions=stats)): forward /
forward_raw return what they return without it, bit for bit, and the frame is added by the blend kernel itself:
per (tile, Gaussian) the wave's totals in a fixed order, then one integer atomic each - a 64-bit add, a 64-bit add of the sum in
fixed point, a 32-bit max of the float's bits.  Integer adds and max commute, so the tensors do not depend on the order in which
tiles, depth chunks or frames arrive: the same frames give the same bits.

The fixed-point sum holds 2^32 units of weight per Gaussian (a full-screen opaque splat over about 2 000 views at 1920x1080)
before it wraps; every (tile, Gaussian) total is truncated below 2^-32.

Statistics frames are rendered without a backward: under torch.no_grad(), or from inputs none of which requires grad.

Error-weighted statistics.  An ErrorStats is a ContributionStats that also scores every Gaussian by the image
error it is responsible for: with a per-pixel error map E in [0, 1] (l1_error_map), E_g = sum over the pixels of w_g E per view.
GaussianRasterizer(settings, contributions=stats, pixel_error=E) takes the fourth total in the same blend kernel and folds the frame
behind its last chunk:

    error_frame_q32 int64   [P]   the running frame's E_g, in units of 2^-32; zero between frames (also behind a frame that raised)
    error_sum_q32   int64   [P]   the sum of E_g over the frames (error_sum: the same as float64) - Taming-3DGS's score
    error_max       float32 [P]   the largest single frame's E_g - the score of "Revising Densification in Gaussian Splatting"

E is read clamped to [0, 1] (a NaN as 0).  A frame without pixel_error leaves the three error tensors alone."""
from __future__ import annotations

import torch

from . import _native as N

Q32 = 2.0 ** -32


class ContributionStats:
    def __init__(self, P: int, device):
        self.P = int(P)
        self.device = torch.device(device)
        if self.P < 0:
            raise ValueError(f"ContributionStats: P = {P}")
        self.count = torch.zeros(self.P, dtype=torch.int64, device=self.device)
        self.weight_sum_q32 = torch.zeros(self.P, dtype=torch.int64, device=self.device)
        self.weight_max = torch.zeros(self.P, dtype=torch.float32, device=self.device)
        self.device = self.count.device              # ("cuda" -> the current device's index)
        self.frames = 0                              # frames accumulated (host side)

    @property
    def weight_sum(self) -> torch.Tensor:
        """float64 [P]: exact, the accumulator has 64 bits and a double's 53 cover 2^21 units of weight at 2^-32."""
        return self.weight_sum_q32.double() * Q32

    def reset(self) -> None:
        self.count.zero_()
        self.weight_sum_q32.zero_()
        self.weight_max.zero_()
        self.frames = 0

    def native(self) -> N.ContribStats:
        """The gsr_contrib_stats of the three tensors (which stay alive with this object)."""
        return N.ContribStats(N._ptr(self.count), N._ptr(self.weight_sum_q32), N._ptr(self.weight_max))

    def __repr__(self):
        return f"ContributionStats(P={self.P}, device={self.device}, frames={self.frames})"


class ErrorStats(ContributionStats):
    def __init__(self, P: int, device):
        super().__init__(P, device)
        self.error_frame_q32 = torch.zeros(self.P, dtype=torch.int64, device=self.device)
        self.error_sum_q32 = torch.zeros(self.P, dtype=torch.int64, device=self.device)
        self.error_max = torch.zeros(self.P, dtype=torch.float32, device=self.device)

    @property
    def error_sum(self) -> torch.Tensor:
        """float64 [P]: exact, as weight_sum."""
        return self.error_sum_q32.double() * Q32

    def reset(self) -> None:
        super().reset()
        self.error_frame_q32.zero_()
        self.error_sum_q32.zero_()
        self.error_max.zero_()

    def native_error(self, pixel_error: torch.Tensor) -> N.ContribError:
        """The gsr_contrib_error of a checked map (check_pixel_error) and this object's frame accumulator."""
        return N.ContribError(N._ptr(pixel_error), N._ptr(self.error_frame_q32))

    def fold(self) -> None:
        """Close a frame on the current stream: error_sum_q32 += error_frame_q32, error_max = max(., its float), error_frame_q32 = 0."""
        with torch.cuda.device(self.device):
            N.contrib_error_fold(self.error_frame_q32, self.error_sum_q32, self.error_max, self.device)

    def __repr__(self):
        return f"ErrorStats(P={self.P}, device={self.device}, frames={self.frames})"


def l1_error_map(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """[H,W]: the per-pixel error map of an image against its target ([C,H,W] each) - the mean absolute difference over the channels,
    clamped to [0, 1].  Plain torch ops on detached values: the map is a weight, never differentiated."""
    with torch.no_grad():
        return (image.detach() - target.detach()).abs().mean(0).clamp(0, 1)


def check_error_stats(stats, what: str) -> None:
    """What a pixel_error asks of `contributions`: that there is one, and that it is an ErrorStats."""
    if stats is None:
        raise ValueError(f"{what}: pixel_error without contributions: the error-weighted total is taken beside the blend statistics "
                         f"(pass an ErrorStats as contributions)")
    if not isinstance(stats, ErrorStats):
        raise ValueError(f"{what}: pixel_error needs contributions to be an ErrorStats, got {type(stats).__name__}")


def check_pixel_error(stats, pixel_error, height: int, width: int, device, what: str) -> torch.Tensor:
    """The refusals of an error frame that need no device -> the map as a contiguous [H,W] tensor."""
    check_error_stats(stats, what)
    if not isinstance(pixel_error, torch.Tensor):
        raise ValueError(f"{what}: pixel_error must be a tensor, got {type(pixel_error).__name__}")
    if pixel_error.dtype != torch.float32:
        raise ValueError(f"{what}: pixel_error must be float32, got {pixel_error.dtype}")
    if tuple(pixel_error.shape) not in ((height, width), (1, height, width)):
        raise ValueError(f"{what}: pixel_error has shape {tuple(pixel_error.shape)}, the frame wants [{height}, {width}] or [1, {height}, {width}]")
    if pixel_error.device != torch.device(device):
        raise ValueError(f"{what}: pixel_error lives on {pixel_error.device}, the inputs on {device}")
    return pixel_error.detach().reshape(height, width).contiguous()


def check_inputs(stats: "ContributionStats", tensors, what: str) -> None:
    """The refusals of a statistics frame that need no device: `stats` is a ContributionStats of the inputs' P and device, and no
    backward can follow (tensors[0] is the positions; None entries are absent optionals)."""
    if not isinstance(stats, ContributionStats):
        raise ValueError(f"{what}: contributions must be a ContributionStats, got {type(stats).__name__}")
    lead = tensors[0]
    if int(lead.shape[0]) != stats.P:
        raise ValueError(f"{what}: contributions holds {stats.P} Gaussians, the inputs {int(lead.shape[0])}")
    if lead.device != stats.device:
        raise ValueError(f"{what}: contributions lives on {stats.device}, the inputs on {lead.device}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise ValueError(f"{what}: a statistics frame has no backward - render it under torch.no_grad() (or from detached inputs)")
