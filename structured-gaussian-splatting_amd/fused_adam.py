"""torch.optim.Adam with the reference's settings (scene/gaussian_model.py:173: lr per group, eps = 1e-15, no weight
decay) whose step is ONE HIP kernel per parameter tensor (csrc/gsr_optim.hip).  State layout ("step",
"exp_avg", "exp_avg_sq") is torch's, so the reference-style optimizer-state surgery (prune / append / replace)
and state_dict round trips work unchanged.

Split groups: a group with `head_cols` = h and `tail` = "<name of another group>" holds tensors [rows, cols, ...]
whose columns [0, h) step with the group's own lr and columns [h, cols) with the lr of the named group, which
itself holds no tensor.  That is how this package's GaussianModel keeps the reference's groups "f_dc"
(lr = feature_lr) and "f_rest" (lr = feature_lr / 20) over ONE interleaved SH table; element for element the
update equals Adam on the two tensors separately.

native=False (and any host tensor) takes the same arithmetic as torch ops, in torch.optim.Adam's own order of
operations (_single_tensor_adam), so CPU runs of the model's host logic agree with torch.optim.Adam bit for bit.
"""
import math

import torch


class FusedAdam(torch.optim.Optimizer):
    bias_correction = True      # SparseFusedAdam can switch it off

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, native=True):
        self.native = native
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    def _tail_lr(self, group):
        for g in self.param_groups:
            if g.get("name") == group["tail"]:
                return float(g["lr"])
        raise KeyError(f"FusedAdam: group {group.get('name')!r} names the tail group {group['tail']!r}, which does not exist")

    @staticmethod
    def _torch_step(p, g, st, step_sizes, b1, b2, eps, step, head_cols):
        m, v = st["exp_avg"], st["exp_avg_sq"]
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / math.sqrt(1 - b2 ** step)).add_(eps)
        if head_cols is None:
            p.addcdiv_(m, denom, value=-step_sizes[0])
        else:
            p[:, :head_cols].addcdiv_(m[:, :head_cols], denom[:, :head_cols], value=-step_sizes[0])
            p[:, head_cols:].addcdiv_(m[:, head_cols:], denom[:, head_cols:], value=-step_sizes[1])

    @torch.no_grad()
    def step(self, closure=None):
        return self._step(closure, None)

    def _step(self, closure, visibility):
        """The step of both classes.  visibility None: every element steps (adam_step_multi); a [P] mask: SparseFusedAdam's step over
        the rows it marks (adam_step_sparse_multi), every parameter being [P, ...]."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        who = "FusedAdam" if visibility is None else "SparseFusedAdam"
        rows = None
        if visibility is not None:
            if visibility.dim() != 1 or visibility.dtype not in (torch.bool, torch.uint8, torch.int32):
                raise TypeError(f"SparseFusedAdam: visibility must be a [P] bool, uint8 or int32 tensor, got {visibility.dtype} "
                                f"{tuple(visibility.shape)}")
            rows = visibility.shape[0]
        seen = None         # the visible rows' indices, for the torch arithmetic of host tensors
        batch = []          # native tensors of this step: ONE launch for all of them (groups that share betas and eps: the reference's do)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            head_cols = group.get("head_cols") if group.get("tail") else None
            lr_tail = self._tail_lr(group) if head_cols is not None else None
            for p in group["params"]:
                if p.grad is None:
                    continue
                if rows is not None and (p.dim() == 0 or p.shape[0] != rows):
                    raise ValueError(f"SparseFusedAdam: group {group.get('name')!r} holds a parameter of shape {tuple(p.shape)}, "
                                     f"the visibility mask has {rows} rows")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                step = int(st["step"])
                lr = float(group["lr"])
                if not (self.native and p.is_cuda):
                    if self.native:
                        raise RuntimeError(f"{who}(native=True) (MI355X build) needs parameters on a HIP device")
                    bc1 = 1 - b1 ** step if self.bias_correction else 1.0
                    args = ((lr / bc1, None if lr_tail is None else lr_tail / bc1), b1, b2, group["eps"],
                            step if self.bias_correction else math.inf, head_cols)
                    if visibility is None:
                        self._torch_step(p, p.grad, st, *args)
                        continue
                    if seen is None:
                        seen = (visibility > 0 if visibility.dtype == torch.int32 else visibility != 0).nonzero().squeeze(1)
                    if seen.numel() == 0:
                        continue
                    # the same arithmetic on copies of the visible rows, written back to them
                    pr = p[seen]
                    rst = {"exp_avg": st["exp_avg"][seen], "exp_avg_sq": st["exp_avg_sq"][seen]}
                    self._torch_step(pr, p.grad[seen], rst, *args)
                    p.index_copy_(0, seen, pr)
                    st["exp_avg"].index_copy_(0, seen, rst["exp_avg"])
                    st["exp_avg_sq"].index_copy_(0, seen, rst["exp_avg_sq"])
                    continue
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                if head_cols is None or p.shape[1] <= head_cols:
                    item = (p, g, st["exp_avg"], st["exp_avg_sq"], lr, lr, step, 0, 0)
                else:
                    width = p.numel() // max(p.shape[0], 1)
                    item = (p, g, st["exp_avg"], st["exp_avg_sq"], lr, lr_tail, step, width, head_cols * (width // p.shape[1]))
                batch.append(((b1, b2, group["eps"], p.device), item))
        if batch:
            from diff_gaussian_rasterization import _native as N
            if not self.bias_correction:
                batch = [(k, it[:6] + (N.ADAM_STEP_UNCORRECTED,) + it[7:]) for k, it in batch]
            while batch:
                key = batch[0][0]
                now = [it for k, it in batch if k == key][:N.ADAM_MAX_TENSORS]
                taken = {id(it[0]) for it in now}
                batch = [(k, it) for k, it in batch if id(it[0]) not in taken]
                if rows == 0:
                    continue
                with torch.cuda.device(key[3]):
                    if visibility is None:
                        N.adam_step_multi(now, *key[:3])
                    else:
                        N.adam_step_sparse_multi(now, visibility, *key[:3])
                for it in now:
                    torch.autograd.graph.increment_version(it[0])    # the kernel wrote through the raw pointer: tell autograd (and
                                                                     # the model's activation cache, which keys on versions)
        return loss


class SparseFusedAdam(FusedAdam):
    """FusedAdam that steps only the rows a frame saw (upstream 3DGS's optimizer_type = "sparse_adam"): step(visibility) takes a
    [P] mask — bool or uint8 (non-zero = visible) or int32 (> 0 = visible: the rasterizer's `radii` as they are) — and updates,
    in ONE launch (k_adam_sparse_multi of csrc/gsr_optim.hip), the visible rows of every parameter [P, ...] that has a gradient.  A hidden row keeps
    its parameter and both moments bit for bit and its gradient is not read.

    state[p]["step"] counts every call in which the tensor had a gradient, whatever the mask showed, and enters the bias corrections
    as in FusedAdam: an all-true mask is FusedAdam's step bit for bit, and the state layout is unchanged.  bias_correction=False
    applies none (step size lr, second moment as it is), which is the arithmetic of upstream's sparse kernel."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, native=True, bias_correction=True):
        self.bias_correction = bool(bias_correction)
        super().__init__(params, lr=lr, betas=betas, eps=eps, native=native)

    @torch.no_grad()
    def step(self, visibility=None, closure=None):
        if visibility is None:
            if not self.bias_correction:
                raise ValueError("SparseFusedAdam(bias_correction=False).step() needs a visibility mask: the dense step is "
                                 "FusedAdam's, which corrects the bias")
            return super().step(closure)
        return self._step(closure, visibility)
