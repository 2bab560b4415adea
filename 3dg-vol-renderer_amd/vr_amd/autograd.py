"""torch.autograd entry point over the mixture queries: the optical depth along rays, differentiable with respect to
the Gaussians' parameters (Device.query_transmittance / Device.query_transmittance_grad) and with respect to the rays
themselves (Device.query_transmittance_ray_grad).

    tau = optical_depth(mean, cov6, density, albedo, origins, directions)      # (n,), on the rays' device
    loss = ((1 - torch.exp(-tau)) - matte).square().sum()                       # alpha mattes, silhouettes, tomography
    loss.backward()                                                             # mean.grad, cov6.grad, density.grad
                                                                                # and, where they require grad,
                                                                                # origins.grad, directions.grad, tmax.grad

Cost: every forward of optical_depth copies the parameters to the host once and builds the scene's tree
(Scene.from_gaussians and an upload). optical_depth_resident is the same function for parameters that live on the
rays' device: its forward hands them to Device.upload_gaussians, which computes records, boxes and the tree on the
device, so nothing is copied to the host and nothing runs per Gaussian on a host thread; it saves the DeviceScene.
tau has the bits of optical_depth's wherever the records' norm words agree (include/vr_hip.h,
vr_upload_gaussians_device: at most 2 ulp apart, on well under 1 % of Gaussians). Either way backward uploads the
saved scene object, which is a no-op while it is the context's current scene, and runs
one gradient query with grad_output as the rays' weights. When origins, directions or a tensor tmax requires grad,
forward runs the ray-gradient query instead of the transmittance query: one walk gives tau (the same bits) and the
seven columns d tau_i / d (origin_i, direction_i, tmax_i), which forward saves and backward multiplies by grad_output.
That is the exact Jacobian product, since tau_i depends on ray i only. The directions are normalised by the library,
so directions.grad is the gradient through v / |v|. Both gradients are exact (closed form, float64 per hit); they are
not differentiable a second time. The optical depth does not depend on albedo, so optical_depth gives it no gradient
(sigma, below, does). When no ray input requires grad, forward and backward issue the calls they issue for the
Gaussians alone.

The optical depth at K distances along each ray (Device.query_transmittance_profile /
Device.query_transmittance_profile_grad): one tree walk per ray in forward, one in backward, whatever K is.

    tau = optical_depth_profile(mean, cov6, density, albedo, origins, directions, t)   # (n, K); t is (K,) or (n, K)
    T = torch.exp(-torch.cat([torch.zeros_like(tau[:, :1]), tau], 1))                   # emission-absorption quadrature:
    x = (origins[:, None] + t_mid[..., None] * directions[:, None]).reshape(-1, 3)      # a sample point per interval
    F, mass = features(mean, cov6, density, albedo, rgb_g, x)                           # (n K, 3), (n K,)
    colour = (F / mass.clamp_min(1e-30)[:, None]).reshape(n, K, 3)                      # the mixture's colour there
    rgb = ((T[:, :-1] - T[:, 1:])[..., None] * colour).sum(1)                           # sum_k (T_k - T_k+1) c_k
    loss.backward()                                                                     # mean.grad, cov6.grad, density.grad,
                                                                                        # rgb_g.grad

optical_depth_profile_resident is the same for parameters on the rays' device. Backward is one profile-gradient call
with grad_output as the (n, K) weights; origins, directions, t and albedo get no gradient.

The caller's own per-Gaussian vectors at points (Device.evaluate_features / Device.features_gradient), the colour of the
quadrature above among them:

    F, mass = features(mean, cov6, density, albedo, feats, points)               # (n, C) = sum_g m_g(x) feats[g], (n,)

feats is (N, C): emission, RGB, SH coefficients, semantic features. features_resident is the same for parameters and
feats on the points' device. Differentiable with respect to mean, cov6, density, feats and points; albedo gets None
(neither output depends on it). Backward is one Device.features_gradient call with (grad_F, grad_mass) as its (weights,
weight_mass), asking only for the outputs some input needs; exact over the forward's active set (float64 per active
Gaussian), the 3-sigma cut-off not differentiated, not differentiable a second time. One profile call plus one feature
call is a differentiable radiance-field renderer on the uploaded tree.

The emission-absorption sum along rays itself, in one call (Device.radiance):

    L, opacity = radiance(mean, cov6, density, albedo, feats, origins, directions, t, q)   # (n, C), (n,)
    loss = (L - image).square().mean()                  # L[i] = sum_k q[i, k] T[i, k] sum_g m_g(x_ik) feats[g]
    loss.backward()                                     # mean.grad, cov6.grad, density.grad, feats.grad

t is (K,) or (n, K), q the quadrature weights in the same shapes or None (ones). The forward is the fused query: it
never holds the n K points or their n K C features, and keeps the (n, K) transmittances for the backward. The
directions are normalised once in torch (v / |v|) and handed over as unit vectors, so that both passes use the same
sample points. The backward composes the gradient queries that exist: one Device.features_gradient at the n K points
with weights q T grad_L and mass weights q T grad_opacity, one Device.evaluate_features for s = grad_L . F + grad_opacity
mass, one Device.query_transmittance_profile_grad with weights -q T s, and the two (N, 10) results added; it asks only
for what some input needs. So the backward costs what the composition costs in memory and walks, and it carries the
feature query's rule that a point whose summed m is <= 0 is zeroed: it is the forward's gradient for positive densities
only. albedo, origins, directions, t and q get None; a fused backward and gradients with respect to the rays are not
part of this.

The same sum with a fused backward (Device.radiance_gradient):

    L, opacity = radiance_fused(mean, cov6, density, albedo, feats, origins, directions, t, q)   # the same forward bits
    loss.backward()                                     # mean.grad, cov6.grad, density.grad, feats.grad and q.grad

radiance_fused and radiance_fused_resident take radiance's arguments. Their backward is one Device.radiance_gradient call
with the saved (n, K) transmittances, asking only for what some input needs: a (ray, Gaussian) pair sums its samples on
chip, and nothing of size n K C or n K 3 is formed. It is the gradient of the forward as defined (every active pair counts,
whatever the sign of the densities), and it also gives q.grad. albedo, origins, directions and t get None.
radiance and radiance_resident stay exactly as they are: existing tests pin their signatures and the sequence of Device
calls their backward makes.

The extinction field itself, at the caller's points (Device.query_sigma / Device.query_sigma_grad):

    sig = sigma(mean, cov6, density, albedo, points)                             # (n, 2) = (sigma_a, sigma_s)
    loss = (sig.sum(1) - grid_density).square().mean()                           # fitting a CT / VDB grid, occupancy and
    loss.backward()                                                              # sparsity terms, sigma_s L of a quadrature
                                                                                 # mean.grad, cov6.grad, density.grad,
                                                                                 # albedo.grad and points.grad

sigma_resident is sigma for parameters on the points' device, as optical_depth_resident is. Backward is one
Device.query_sigma_grad call with grad_output as the (w_a, w_s) weights; it asks for the Gaussians' rows only when a
parameter requires grad and for the points' rows only when points does. The gradient is that of sigma_s = sum alpha m,
sigma_a = sum (1 - alpha) m over the forward's active set (exact, float64 per active Gaussian); the 3-sigma cut-off is
not differentiated, and the result is not differentiable a second time.
"""
import numpy as np
import torch

from . import Device, Scene


def _scene_of(mean, cov6, density, albedo, batch, what, device, resident):
    """(Device, scene) of a forward: the parameters uploaded from where they are (resident: they must be on the device
    of `batch`, "the rays" or "the points") or through a host Scene."""
    params = (mean, cov6, density, albedo)
    if resident:
        for t, name in zip(params, ("mean", "cov6", "density", "albedo")):
            if t.device != batch.device:
                raise ValueError(f"{name} is on {t.device}, {what} on {batch.device}: a resident scene's "
                                 f"parameters live on {what}' device")
    dev = Device.get(device)
    if resident:
        return dev, dev.upload_gaussians(*(t.detach().to(torch.float32).contiguous() for t in params))
    return dev, Scene.from_gaussians(*(t.detach().to("cpu", torch.float32).contiguous().numpy() for t in params))


def _split_grad(g, like, needs):
    """The (N, 10 or 11) gradient g as one tensor per parameter in `like` (mean, cov6, density[, albedo]), shaped and
    typed as it; None where `needs` says no gradient is wanted."""
    cols = (g[:, 0:3], g[:, 3:9], g[:, 9], g[:, 10:11])
    return tuple(x.reshape(p.shape).to(device=p.device, dtype=p.dtype) if need else None for x, p, need in zip(cols, like, needs))


class _OpticalDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, origins, directions, tmax, device, moving_bounds, resident=False):
        dev, scene = _scene_of(mean, cov6, density, albedo, origins, "the rays", device, resident)
        o, d = origins.detach().contiguous(), directions.detach().contiguous()
        tm = tmax.detach() if torch.is_tensor(tmax) else float(tmax)
        ctx.ray_needs = tuple(ctx.needs_input_grad[4:7])
        ctx.ray_jac = None
        if any(ctx.ray_needs):
            g_o, g_d, g_t, tau = dev.query_transmittance_ray_grad(scene, o, d, tm, moving_bounds=bool(moving_bounds))
            ctx.ray_jac = (g_o, g_d, g_t)
            tau = tau.contiguous()
        else:
            _, tau = dev.query_transmittance(scene, o, d, tm, return_tau=True)
        ctx.dev, ctx.scene, ctx.rays, ctx.moving = dev, scene, (o, d, tm), bool(moving_bounds)
        ctx.like = (mean, cov6, density)
        ctx.ray_like = tuple((tuple(t.shape), t.dtype) if torch.is_tensor(t) else None for t in (origins, directions, tmax))
        return tau

    @staticmethod
    def backward(ctx, grad_tau):
        o, d, tm = ctx.rays
        out = (None,) * 3
        if ctx.ray_jac is None or any(ctx.needs_input_grad[:3]):
            g = ctx.dev.query_transmittance_grad(ctx.scene, o, d, grad_tau.to(torch.float32).contiguous(), tm,
                                                 moving_bounds=ctx.moving)
            out = _split_grad(g, ctx.like, ctx.needs_input_grad[:3])
        rays = [None, None, None]
        if ctx.ray_jac is not None:
            g_o, g_d, g_t = ctx.ray_jac
            gt = grad_tau.to(torch.float32)
            if ctx.ray_needs[0]:
                rays[0] = (g_o * gt[:, None]).to(ctx.ray_like[0][1])
            if ctx.ray_needs[1]:
                rays[1] = (g_d * gt[:, None]).to(ctx.ray_like[1][1])
            if ctx.ray_needs[2]:  # (one tmax for all rays: the sum over the rays)
                shape, dtype = ctx.ray_like[2]
                gtm = g_t * gt
                rays[2] = (gtm if gtm.numel() == int(np.prod(shape)) else gtm.sum()).reshape(shape).to(dtype)
        return out + (None,) + tuple(rays) + (None, None, None)


def optical_depth(mean, cov6, density, albedo, origins, directions, tmax=float("inf"), device=0, moving_bounds=True):
    """tau (n,) float32 along rays (origins, directions: (n, 3) float32 tensors on cuda:`device`; tmax a number or an
    (n,) tensor there) through the mixture of Gaussians mean (N, 3), cov6 (N, 6) [xx xy xz yy yz zz], density (N,),
    albedo (N,) (tensors on any device). Differentiable with respect to mean, cov6 and density, and with respect to
    origins, directions (through the library's normalisation v / |v|) and a tensor tmax; the other arguments get
    None. moving_bounds=False differentiates with each Gaussian's 3-sigma entry / exit distances held fixed."""
    return _OpticalDepth.apply(mean, cov6, density, albedo, origins, directions, tmax, device, moving_bounds, False)


def optical_depth_resident(mean, cov6, density, albedo, origins, directions, tmax=float("inf"), device=0, moving_bounds=True):
    """optical_depth for parameters that never leave the GPU: mean, cov6, density and albedo must be on the rays'
    device (ValueError otherwise), and forward uploads them with Device.upload_gaussians instead of copying them to
    the host. Same arguments, same gradients."""
    return _OpticalDepth.apply(mean, cov6, density, albedo, origins, directions, tmax, device, moving_bounds, True)


class _OpticalDepthProfile(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, origins, directions, t, device, moving_bounds, resident):
        dev, scene = _scene_of(mean, cov6, density, albedo, origins, "the rays", device, resident)
        o, d, ts = origins.detach().contiguous(), directions.detach().contiguous(), t.detach().contiguous()
        _, tau = dev.query_transmittance_profile(scene, o, d, ts, return_tau=True)
        ctx.dev, ctx.scene, ctx.rays, ctx.moving = dev, scene, (o, d, ts), bool(moving_bounds)
        ctx.like = (mean, cov6, density)
        return tau

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_tau):
        o, d, ts = ctx.rays
        out = (None,) * 3
        if any(ctx.needs_input_grad[:3]):
            g = ctx.dev.query_transmittance_profile_grad(ctx.scene, o, d, ts, grad_tau.to(torch.float32).contiguous(),
                                                         moving_bounds=ctx.moving)
            out = _split_grad(g, ctx.like, ctx.needs_input_grad[:3])
        return out + (None,) * 7


def optical_depth_profile(mean, cov6, density, albedo, origins, directions, t, device=0, moving_bounds=True):
    """tau (n, K) float32: the optical depth at the distances t ((K,) shared by all rays, or (n, K); a float32 tensor on
    cuda:`device`, in any order) along rays (origins, directions: (n, 3) float32 tensors there) through the mixture of
    Gaussians mean (N, 3), cov6 (N, 6) [xx xy xz yy yz zz], density (N,), albedo (N,) (tensors on any device). Column k
    has the bits of optical_depth(..., tmax=t[:, k]). Differentiable with respect to mean, cov6 and density: backward
    is one Device.query_transmittance_profile_grad call with grad_output as the weights. origins, directions, t and
    albedo get None (the profile's gradient with respect to the rays and the distances is not computed).
    moving_bounds=False differentiates with each Gaussian's 3-sigma entry / exit distances held fixed."""
    return _OpticalDepthProfile.apply(mean, cov6, density, albedo, origins, directions, t, device, moving_bounds, False)


def optical_depth_profile_resident(mean, cov6, density, albedo, origins, directions, t, device=0, moving_bounds=True):
    """optical_depth_profile for parameters that never leave the GPU: mean, cov6, density and albedo must be on the
    rays' device (ValueError otherwise), and forward uploads them with Device.upload_gaussians instead of copying them
    to the host. Same arguments, same gradients; origins, directions, t and albedo get None."""
    return _OpticalDepthProfile.apply(mean, cov6, density, albedo, origins, directions, t, device, moving_bounds, True)


class _Sigma(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, points, device, resident):
        dev, scene = _scene_of(mean, cov6, density, albedo, points, "the points", device, resident)
        pts = points.detach().contiguous()
        ctx.dev, ctx.scene, ctx.pts = dev, scene, pts
        ctx.like = (mean, cov6, density, albedo)
        ctx.pts_dtype = points.dtype
        return dev.query_sigma(scene, pts)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sigma):
        need_g, need_x = any(ctx.needs_input_grad[:4]), ctx.needs_input_grad[4]
        out, gx = (None,) * 4, None
        if need_g or need_x:
            got = ctx.dev.query_sigma_grad(ctx.scene, ctx.pts, grad_sigma.to(torch.float32).contiguous(),
                                           gaussians=need_g, positions=need_x)
            g, gx = got if need_g and need_x else (got, None) if need_g else (None, got)
            if need_g:
                out = _split_grad(g, ctx.like, ctx.needs_input_grad[:4])
            if need_x:
                gx = gx.to(ctx.pts_dtype)
        return out + (gx, None, None)


def sigma(mean, cov6, density, albedo, points, device=0):
    """sigma (n, 2) float32 = (sigma_a, sigma_s) at points ((n, 3) float32 tensor on cuda:`device`) of the mixture of
    Gaussians mean (N, 3), cov6 (N, 6) [xx xy xz yy yz zz], density (N,), albedo (N,) (tensors on any device): the values
    of Device.query_sigma. Differentiable with respect to mean, cov6, density, albedo and points."""
    return _Sigma.apply(mean, cov6, density, albedo, points, device, False)


def sigma_resident(mean, cov6, density, albedo, points, device=0):
    """sigma for parameters that never leave the GPU: mean, cov6, density and albedo must be on the points' device
    (ValueError otherwise), and forward uploads them with Device.upload_gaussians instead of copying them to the
    host. Same arguments, same gradients."""
    return _Sigma.apply(mean, cov6, density, albedo, points, device, True)


class _Features(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, feats, points, device, resident):
        if resident and feats.device != points.device:
            raise ValueError(f"feats is on {feats.device}, the points on {points.device}: a resident scene's "
                             "features live on the points' device")
        dev, scene = _scene_of(mean, cov6, density, albedo, points, "the points", device, resident)
        pts = points.detach().contiguous()
        f = feats.detach().to(device=pts.device, dtype=torch.float32).contiguous()
        ctx.dev, ctx.scene, ctx.pts, ctx.f = dev, scene, pts, f
        ctx.like = (mean, cov6, density)
        ctx.feats_like, ctx.pts_dtype = feats, points.dtype
        F, mass = dev.evaluate_features(scene, pts, f, return_mass=True)
        return F, mass

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_F, grad_mass):
        need_g, need_f, need_x = any(ctx.needs_input_grad[:3]), ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        out, gf, gx = (None,) * 3, None, None
        if need_g or need_f or need_x:
            got = ctx.dev.features_gradient(ctx.scene, ctx.pts, ctx.f, grad_F.to(torch.float32).contiguous(),
                                              grad_mass.to(torch.float32).contiguous(), gaussians=need_g, features_grad=need_f,
                                              positions=need_x)
            got = list(got) if isinstance(got, tuple) else [got]
            if need_g:
                out = _split_grad(got.pop(0), ctx.like, ctx.needs_input_grad[:3])
            if need_f:
                gf = got.pop(0).to(device=ctx.feats_like.device, dtype=ctx.feats_like.dtype)
            if need_x:
                gx = got.pop(0).to(ctx.pts_dtype)
        return out + (None, gf, gx, None, None)


def features(mean, cov6, density, albedo, feats, points, device=0):
    """(F (n, C), mass (n,)) float32 at points ((n, 3) float32 tensor on cuda:`device`): F[i, c] = sum_g m_g(x_i) feats[g, c]
    and mass[i] = sum_g m_g(x_i) over the Gaussians active at x_i, for the mixture mean (N, 3), cov6 (N, 6) [xx xy xz yy yz
    zz], density (N,), albedo (N,) and the caller's feats (N, C) (tensors on any device): the values of
    Device.evaluate_features. Differentiable with respect to mean, cov6, density, feats and points; albedo gets None."""
    return _Features.apply(mean, cov6, density, albedo, feats, points, device, False)


def features_resident(mean, cov6, density, albedo, feats, points, device=0):
    """features for parameters that never leave the GPU: mean, cov6, density, albedo and feats must be on the points'
    device (ValueError otherwise), and forward uploads the scene with Device.upload_gaussians instead of copying it to the
    host. Same arguments, same gradients."""
    return _Features.apply(mean, cov6, density, albedo, feats, points, device, True)


def _unit_directions(d):
    """v / |v| per row in f32, |v|^2 summed as the library sums it."""
    s = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d / torch.sqrt(s)[:, None]).contiguous()


class _Radiance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, feats, origins, directions, t, q, device, resident):
        if resident and feats.device != origins.device:
            raise ValueError(f"feats is on {feats.device}, the rays on {origins.device}: a resident scene's "
                             "features live on the rays' device")
        dev, scene = _scene_of(mean, cov6, density, albedo, origins, "the rays", device, resident)
        o, d = origins.detach().contiguous(), _unit_directions(directions.detach())
        ts = t.detach().contiguous()
        qs = None if q is None else q.detach().contiguous()
        f = feats.detach().to(device=o.device, dtype=torch.float32).contiguous()
        L, opacity, tr = dev.radiance(scene, o, d, ts, f, qs, unit=True, return_opacity=True, return_tr=True)
        ctx.dev, ctx.scene, ctx.saved = dev, scene, (o, d, ts, qs, f, tr)
        ctx.like, ctx.feats_like = (mean, cov6, density), feats
        ctx.mark_non_differentiable(tr)
        return L, opacity, tr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_L, grad_opacity, _grad_tr):
        need_g, need_f = any(ctx.needs_input_grad[:3]), ctx.needs_input_grad[4]
        out, gf = (None,) * 3, None
        if need_g or need_f:
            o, d, ts, qs, f, tr = ctx.saved
            n, K = tr.shape
            C = f.shape[1]
            # the weights are formed in double and rounded once, so they carry one f32 rounding each
            gL, gA = grad_L.to(torch.float64), grad_opacity.to(torch.float64)
            tk = ts.expand(n, K)
            x = (o[:, None, :] + tk[:, :, None] * d[:, None, :]).reshape(-1, 3).contiguous()
            valid = torch.isfinite(tk) & (tk >= 0) & torch.isfinite(tr)  # (an invalid ray's T is NaN: it contributes nothing)
            qt = tr.to(torch.float64) if qs is None else qs.expand(n, K).to(torch.float64) * tr.to(torch.float64)  # (n, K): q T
            qt = torch.where(valid, qt, torch.zeros_like(qt))
            x = torch.where(valid.reshape(-1, 1), x, torch.full_like(x, float("nan")))  # (a non-finite point lies in no box)
            w = (qt[:, :, None] * gL[:, None, :]).reshape(-1, C).to(torch.float32).contiguous()
            u = (qt * gA[:, None]).reshape(-1).to(torch.float32).contiguous()
            got = ctx.dev.features_gradient(ctx.scene, x, f, w, u, gaussians=need_g, features_grad=need_f)
            got = list(got) if isinstance(got, tuple) else [got]
            if need_g:
                g = got.pop(0)
                F, mass = ctx.dev.evaluate_features(ctx.scene, x, f, return_mass=True)
                s = (F.reshape(n, K, C).to(torch.float64) * gL[:, None, :]).sum(2) + mass.reshape(n, K).to(torch.float64) * gA[:, None]
                wp = torch.where(valid, -qt * s, torch.zeros_like(s)).to(torch.float32).contiguous()
                gp = ctx.dev.query_transmittance_profile_grad(ctx.scene, o, d, ts, wp)
                out = _split_grad(g.to(torch.float64) + gp.to(torch.float64), ctx.like, ctx.needs_input_grad[:3])
            if need_f:
                gf = got.pop(0).to(device=ctx.feats_like.device, dtype=ctx.feats_like.dtype)
        return out + (None, gf) + (None,) * 6


def radiance(mean, cov6, density, albedo, feats, origins, directions, t, q=None, device=0):
    """(L (n, C), opacity (n,)) float32 along rays (origins, directions: (n, 3) float32 tensors on cuda:`device`) at the
    distances t ((K,) shared by all rays, or (n, K)) with the quadrature weights q (t's shapes, or None: ones), for the
    mixture mean (N, 3), cov6 (N, 6) [xx xy xz yy yz zz], density (N,), albedo (N,) and the caller's feats (N, C) (tensors on
    any device): L[i] = sum_k q[i, k] T[i, k] sum_g m_g(x_ik) feats[g], opacity the same sum without feats; the values of
    Device.radiance for the directions normalised in torch and unit=True. Differentiable with respect to mean, cov6,
    density and feats (positive densities; see the module's head); albedo, origins, directions, t and q get None."""
    L, opacity, _ = _Radiance.apply(mean, cov6, density, albedo, feats, origins, directions, t, q, device, False)
    return L, opacity


def radiance_resident(mean, cov6, density, albedo, feats, origins, directions, t, q=None, device=0):
    """radiance for parameters that never leave the GPU: mean, cov6, density, albedo and feats must be on the rays' device
    (ValueError otherwise), and forward uploads the scene with Device.upload_gaussians instead of copying it to the host.
    Same arguments, same gradients."""
    L, opacity, _ = _Radiance.apply(mean, cov6, density, albedo, feats, origins, directions, t, q, device, True)
    return L, opacity


class _RadianceFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, cov6, density, albedo, feats, origins, directions, t, q, device, resident):
        if resident and feats.device != origins.device:
            raise ValueError(f"feats is on {feats.device}, the rays on {origins.device}: a resident scene's "
                             "features live on the rays' device")
        dev, scene = _scene_of(mean, cov6, density, albedo, origins, "the rays", device, resident)
        o, d = origins.detach().contiguous(), _unit_directions(directions.detach())
        ts = t.detach().contiguous()
        qs = None if q is None else q.detach().contiguous()
        f = feats.detach().to(device=o.device, dtype=torch.float32).contiguous()
        L, opacity, tr = dev.radiance(scene, o, d, ts, f, qs, unit=True, return_opacity=True, return_tr=True)
        ctx.dev, ctx.scene, ctx.saved = dev, scene, (o, d, ts, qs, f, tr)
        ctx.like, ctx.feats_like, ctx.q_like = (mean, cov6, density), feats, q
        ctx.mark_non_differentiable(tr)
        return L, opacity, tr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_L, grad_opacity, _grad_tr):
        need_g, need_f = any(ctx.needs_input_grad[:3]), ctx.needs_input_grad[4]
        need_q = ctx.q_like is not None and ctx.needs_input_grad[8]
        out, gf, gq = (None,) * 3, None, None
        if need_g or need_f or need_q:
            o, d, ts, qs, f, tr = ctx.saved
            got = ctx.dev.radiance_gradient(ctx.scene, o, d, ts, f, grad_L.to(torch.float32).contiguous(),
                                            grad_opacity.to(torch.float32).contiguous(), qs, tr, unit=True,
                                            gaussians=need_g, features_grad=need_f, grad_q=need_q)
            got = list(got) if isinstance(got, tuple) else [got]
            if need_g:
                out = _split_grad(got.pop(0), ctx.like, ctx.needs_input_grad[:3])
            if need_f:
                gf = got.pop(0).to(device=ctx.feats_like.device, dtype=ctx.feats_like.dtype)
            if need_q:
                gq = got.pop(0)
                if ctx.q_like.dim() == 1:  # (one row shared by all rays: the sum over the rays)
                    gq = gq.sum(0)
                gq = gq.to(ctx.q_like.dtype)
        return out + (None, gf, None, None, None, gq, None, None)


def radiance_fused(mean, cov6, density, albedo, feats, origins, directions, t, q=None, device=0):
    """radiance with a fused backward: the same arguments and the same (L, opacity) bits. Backward is one
    Device.radiance_gradient call with the forward's transmittances; differentiable with respect to mean, cov6, density, feats
    and q (a shared (K,) row gets the sum over the rays); albedo, origins, directions and t get None."""
    L, opacity, _ = _RadianceFused.apply(mean, cov6, density, albedo, feats, origins, directions, t, q, device, False)
    return L, opacity


def radiance_fused_resident(mean, cov6, density, albedo, feats, origins, directions, t, q=None, device=0):
    """radiance_fused for parameters that never leave the GPU: mean, cov6, density, albedo and feats must be on the rays'
    device (ValueError otherwise), and forward uploads the scene with Device.upload_gaussians. Same arguments, same gradients."""
    L, opacity, _ = _RadianceFused.apply(mean, cov6, density, albedo, feats, origins, directions, t, q, device, True)
    return L, opacity
