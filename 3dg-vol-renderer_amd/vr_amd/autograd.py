"""torch.autograd entry point over the mixture queries: the optical depth along known rays, differentiable with respect
to the Gaussians' parameters (Device.query_transmittance / Device.query_transmittance_grad).

    tau = optical_depth(mean, cov6, density, albedo, origins, directions)      # (n,), on the rays' device
    loss = ((1 - torch.exp(-tau)) - matte).square().sum()                       # alpha mattes, silhouettes, tomography
    loss.backward()                                                             # mean.grad, cov6.grad, density.grad

Cost: every forward copies the parameters to the host once and builds the scene's tree (Scene.from_gaussians and an
upload); backward uploads the same scene object, which is a no-op while it is the context's current scene, and runs
one gradient query with grad_output as the rays' weights. The gradient is exact (closed form, float64 per hit); it is
not differentiable a second time, and no gradient flows to the rays, tmax or albedo.
"""
import numpy as np
import torch

from . import Device, Scene


class _OpticalDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, origins, directions, tmax, device, moving_bounds):
        dev = Device.get(device)
        host = [t.detach().to("cpu", torch.float32).contiguous().numpy() for t in (mean, cov6, density, albedo)]
        scene = Scene.from_gaussians(*host)
        o, d = origins.detach().contiguous(), directions.detach().contiguous()
        tm = tmax.detach() if torch.is_tensor(tmax) else float(tmax)
        _, tau = dev.query_transmittance(scene, o, d, tm, return_tau=True)
        ctx.dev, ctx.scene, ctx.rays, ctx.moving = dev, scene, (o, d, tm), bool(moving_bounds)
        ctx.like = (mean, cov6, density)
        return tau

    @staticmethod
    def backward(ctx, grad_tau):
        o, d, tm = ctx.rays
        g = ctx.dev.query_transmittance_grad(ctx.scene, o, d, grad_tau.to(torch.float32).contiguous(), tm,
                                             moving_bounds=ctx.moving)
        mean, cov6, density = ctx.like
        out = (g[:, 0:3].reshape(mean.shape), g[:, 3:9].reshape(cov6.shape), g[:, 9].reshape(density.shape))
        out = tuple(x.to(device=p.device, dtype=p.dtype) if need else None
                    for x, p, need in zip(out, ctx.like, ctx.needs_input_grad[:3]))
        return out + (None,) * 6


def optical_depth(mean, cov6, density, albedo, origins, directions, tmax=float("inf"), device=0, moving_bounds=True):
    """tau (n,) float32 along rays (origins, directions: (n, 3) float32 tensors on cuda:`device`; tmax a number or an
    (n,) tensor there) through the mixture of Gaussians mean (N, 3), cov6 (N, 6) [xx xy xz yy yz zz], density (N,),
    albedo (N,) (tensors on any device). Differentiable with respect to mean, cov6 and density; the other arguments
    get None. moving_bounds=False differentiates with each Gaussian's 3-sigma entry / exit distances held fixed."""
    return _OpticalDepth.apply(mean, cov6, density, albedo, origins, directions, tmax, device, moving_bounds)
