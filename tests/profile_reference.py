"""Reference model of the profile gradient query (Device.query_transmittance_profile_grad): grad_reference.Model on the
n * K expanded rays (ray i, tmax = t[i, k], weight[i, k]), with the oracle's probe taken once per ray instead of once per
expanded ray: the probe (intersect_direct's f32 t_enter / t_exit) depends on the ray alone, not on tmax. Everything else
is grad_reference's: column k is R.Model's arithmetic for tmax = t[:, k], line for line, through R.contributions.
test_gpu_query_profile.py checks the 1_gaussian cases against a literal R.Model of the expanded rays. Computed once per
case, shared, never modified."""
import numpy as np

import grad_reference as R


class ProfileModel:
    def __init__(self, sc, o, d, t):
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        n = len(o)
        t = np.asarray(t, np.float32)
        self.t = np.broadcast_to(t, (n, t.shape[-1])).copy()
        self.K = self.t.shape[1]
        hit, te, tx = R.probe(sc, o, d)
        rec = sc.records().astype(np.float64)
        self.N = rec.shape[0]
        mean, rho, norm, M = rec[:, :3], rec[:, 3], rec[:, 10], R.sym(rec[:, 4:10])
        with np.errstate(invalid="ignore"):
            dn = R.normalized_f32(d)
        ray_ok = np.isfinite(o).all(1) & np.isfinite(dn).all(1)
        self.hit, self.te, self.tx, self.ray_ok = hit, te, tx, ray_ok
        self.use, self._frozen, self._moving = [], [], []
        for k in range(self.K):
            tmax = self.t[:, k]
            with np.errstate(invalid="ignore"):
                a = np.maximum(np.float32(0), te)  # f32, as the device clips
                b = np.minimum(tmax[:, None], tx)
                valid = ray_ok & (tmax > 0)
            use = hit & (b > a) & valid[:, None]
            o64 = np.where(valid[:, None], o, 0.0).astype(np.float64)
            d64 = np.where(valid[:, None], dn, np.float32([1, 0, 0])).astype(np.float64)
            a64, b64 = np.where(use, a, 0.0).astype(np.float64), np.where(use, b, 1.0).astype(np.float64)
            args = (mean, M, norm, rho, o64, d64, a64, b64, use)
            self.use.append(use)
            self._frozen.append(R.contributions(*args, np.zeros_like(use), np.zeros_like(use)))
            self._moving.append(R.contributions(*args, use & (te > 0), use & (tx <= tmax[:, None])))
        for x in self._frozen + self._moving:
            x.setflags(write=False)

    def classes(self):
        """Numbers of (ray, sample, Gaussian) triples of hit Gaussians on valid rays with the sample before the entry
        (or not > 0), strictly inside the chord, and at or past the exit."""
        a = np.maximum(np.float32(0), self.te)[:, None, :]
        t = self.t[:, :, None]
        hit = (self.hit & self.ray_ok[:, None])[:, None, :]
        with np.errstate(invalid="ignore"):
            before, inside, past = hit & ~(t > a), hit & (t > a) & (t < self.tx[:, None, :]), hit & (t >= self.tx[:, None, :]) & (t > a)
        return int(before.sum()), int(inside.sum()), int(past.sum())

    def grad(self, weights=None, moving=True, cols=None):
        """(G64, S), each (N, 10): sum_i sum_k w[i, k] contribution and the sum of the absolute values, over columns `cols`."""
        c = self._moving if moving else self._frozen
        w = np.ones((len(self.t), self.K)) if weights is None else np.asarray(weights, np.float64)
        G, S = np.zeros((self.N, 10)), np.zeros((self.N, 10))
        for k in (range(self.K) if cols is None else cols):
            term = c[k] * w[:, k, None, None]
            G += term.sum(0)
            S += np.abs(term).sum(0)
        return G, S
