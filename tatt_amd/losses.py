"""The losses and the rotation augmentation around the SR generator, as the reference's training loop uses them
 -- same class names, constructor arguments and call signatures, HIP kernels underneath:

    ImageLoss(gradient=True, loss_weight=[1, 1e-4])      reference loss/image_loss.py:9-34
    SemanticLoss()                                       reference loss/semantic_loss.py:7-38
    SSIM(window_size=11, size_average=True)              reference utils/ssim_psnr.py:202-228   (first 3 channels)
    TRI_SSIM(window_size=11, size_average=True)          reference utils/ssim_psnr.py:231-256   (all channels)
    calculate_psnr(img1, img2)                           reference utils/ssim_psnr.py:9-15
    CTCLoss(blank=0, reduction='mean', zero_infinity=False)   torch.nn.CTCLoss, reference interfaces/super_resolution.py:51
    ctc_loss_from_logits(logits, codes, lengths, ...)    the same loss on raw logits, log-softmax fused (the training step's form)
    torch_distortion(images, arcs, rand_offs)            reference model/__init__.py:4-29 (= TextSR.torch_rotate_img)

No CPU fallback: tensors must live on an AMD GPU.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import functional as Fh
from .train import calculate_psnr, ctc_loss_from_logits, image_loss, semantic_loss  # noqa: F401  (re-exported)
from .train import _ctc_reduce, _ctc_row_offsets


class ImageLoss(nn.Module):
    def __init__(self, gradient=True, loss_weight=(20, 1e-4)):
        super().__init__()
        self.gradient = gradient
        self.loss_weight = list(loss_weight)

    def forward(self, out_images, target_images, grad_mask=None):
        # grad_mask: accepted and ignored, exactly as the reference does (loss/image_loss.py:19-23 never reads it)
        w1 = float(self.loss_weight[1]) if self.gradient else 0.0
        return image_loss(out_images, target_images, (float(self.loss_weight[0]), w1))


class SemanticLoss(nn.Module):
    def forward(self, pred_vec, gt_vec):
        return semantic_loss(pred_vec, gt_vec)


class _SsimBase(nn.Module):
    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        if window_size != 11:
            # documented limit: every call site of the reference constructs SSIM() / TRI_SSIM() with the default
            raise NotImplementedError("the HIP SSIM kernels implement the 11x11 window every reference call site uses")
        self.window_size, self.size_average = window_size, size_average

    def _reduce(self, per_sample):
        # size_average: mean over every element == mean of the per-sample means (equal counts); else the reference's
        # .mean(1).mean(1).mean(1) per sample
        return per_sample.mean() if self.size_average else per_sample


class SSIM(_SsimBase):
    def forward(self, img1, img2):
        return self._reduce(Fh.SsimFn.apply(img1[:, :3], img2[:, :3], None))


class TRI_SSIM(_SsimBase):
    def forward(self, img1, img2, img3):
        return self._reduce(Fh.SsimFn.apply(img1, img2, img3))


class CTCLoss(nn.Module):
    """torch.nn.CTCLoss with the same constructor and call: `forward(log_probs (T,B,C) or (T,C), targets, input_lengths,
    target_lengths)`, targets padded (B, S) or concatenated 1-D, lengths as tensors (host or device) or sequences of ints.  One HIP
    launch computes the losses and the gradient (tatt_ctc_loss_fwd); label data that lives on the host goes to the device with
    non-blocking copies and is never read back, so the call does not wait for the GPU.  What torch rejects on the host cannot be
    rejected here without reading the lengths: an input length outside [0, T] makes its sample infeasible (inf, or 0 with
    zero_infinity), and a NEGATIVE target length marks a sample to be ignored (loss and gradient 0)."""

    def __init__(self, blank: int = 0, reduction: str = "mean", zero_infinity: bool = False):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError("reduction must be 'none', 'mean' or 'sum', got %r" % (reduction,))
        self.blank, self.reduction, self.zero_infinity = int(blank), reduction, bool(zero_infinity)

    @staticmethod
    def _i32(v, dev):
        t = v if isinstance(v, torch.Tensor) else torch.tensor(list(v) if not isinstance(v, int) else [v], dtype=torch.int32)
        if t.is_cuda:
            return t.to(device=dev, dtype=torch.int32).contiguous()
        return t.to(torch.int32).contiguous().pin_memory().to(dev, non_blocking=True)

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        Fh.ops._check_dev(log_probs)
        dev = log_probs.device
        if log_probs.dim() == 2:                                  # unbatched (T, C): one sample, targets (S,)
            log_probs = log_probs.unsqueeze(1)
            if isinstance(targets, torch.Tensor):
                targets = targets.reshape(1, -1)
        B = log_probs.shape[1]
        codes = self._i32(targets, dev)
        tl = self._i32(target_lengths, dev).reshape(-1)
        il = self._i32(input_lengths, dev).reshape(-1)
        if codes.dim() == 2:
            offs = _ctc_row_offsets(B, codes.shape[1], dev)
        else:                                                     # torch's concatenated form: exclusive prefix sum of the lengths
            pos = tl.clamp_min(0)
            offs = torch.cumsum(pos, 0, dtype=torch.int32) - pos
        nll = Fh.CtcLossFn.apply(log_probs, codes, offs, tl, il, self.blank, self.zero_infinity, True)
        return _ctc_reduce(nll, tl, self.reduction)


def rotation_theta(arcs: torch.Tensor, rand_offs: torch.Tensor, H: int, W: int, off_range: float = 0.2) -> torch.Tensor:
    """The (N,2,3) affine matrices of torch_distortion (reference model/__init__.py:9-26): rotation by `arcs` with the aspect
    ratio H/W jittered by `rand_offs`.  Plain torch arithmetic on whatever device the inputs live on (N numbers)."""
    arcs, rand_offs = arcs.float(), rand_offs.float()
    rm = H / float(W) + rand_offs * off_range * 2 - off_range
    cos, sin, zero = torch.cos(arcs), torch.sin(arcs), torch.zeros_like(arcs)
    return torch.stack([cos, sin * rm, zero, -sin / rm, cos, zero], 1).reshape(-1, 2, 3)


def torch_distortion(torch_image_batches, arc_batches, rand_offs, off_range=0.2):
    N, C, H, W = torch_image_batches.shape
    theta = rotation_theta(arc_batches, rand_offs, H, W, off_range)
    return Fh.AffineSampleFn.apply(torch_image_batches, theta)


