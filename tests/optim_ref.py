"""NumPy mirrors of the six update rules of 001_train_autoencoder/misc/optim_updates.lua as nvqa_optim_update applies them:
clamp -> weight decay -> the rule, with the log line's two statistics, state held in `dtype` (float32 = the device's
arithmetic, float64 = the yardstick of the float32 mirror's own rounding).  wd_first=True is the order of the weak-paired
script's cnn branch (nvqa_ae_wp_projection_update): weight decay, then the clamp.  In the style of ae_ref_torch.Adam; the
equations are restated here, nothing is taken from the library.

    sgd      x <- x - lr g
    sgdm     v <- a v + lr g;                 x <- x - v
    sgdmom   m' <- a m - lr g;                x <- x - a m + (1 + a) m'
    adagrad  m <- m + g g;                    x <- x - lr g / (sqrt(m) + eps)
    rmsprop  m <- a m + (1 - a) g g;          x <- x - lr g / (sqrt(m) + eps)
    adam     m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g g;  t <- t + 1
             x <- x - lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)
"""
import numpy as np

SGD, SGDM, SGDMOM, ADAGRAD, RMSPROP, ADAM = range(6)
NAMES = {SGD: "sgd", SGDM: "sgdm", SGDMOM: "sgdmom", ADAGRAD: "adagrad", RMSPROP: "rmsprop", ADAM: "adam"}


class Optim:
    def __init__(self, rule, n, dtype=np.float32, wd_first=False):
        assert rule in NAMES
        self.rule, self.f, self.wd_first = rule, dtype, wd_first
        self.m = np.zeros(n, dtype)
        self.v = np.zeros(n, dtype)
        self.t = 0

    def update(self, x, g, lr, alpha=0.8, beta=0.999, eps=1e-8, wd=0.0, clamp=0.0):
        """returns (new x, paramsNorm, # updates) -- the statistics of x before the update, g after clamp and weight decay"""
        f32 = np.float32  # the device takes its scalars as floats: the float64 mirror starts from the same values
        f = lambda v: self.f(f32(v))  # noqa: E731
        x, g = np.asarray(x, self.f), np.asarray(g, self.f)
        if self.wd_first and wd != 0:
            g = (g + f(wd) * x).astype(self.f)
        if clamp > 0:
            g = np.clip(g, f(-clamp), f(clamp))
        if not self.wd_first and wd != 0:
            g = (g + f(wd) * x).astype(self.f)
        norm = float(np.sqrt((x.astype(np.float64) ** 2).sum()))
        count = int((np.abs(g * f(lr)) >= np.abs(x) * f(0.01)).sum())
        a, b, r = f(alpha), f(beta), self.rule
        if r == SGD:
            x = x - f(lr) * g
        elif r == SGDM:
            self.m = (a * self.m + f(lr) * g).astype(self.f)
            x = x - self.m
        elif r == SGDMOM:
            m0 = self.m
            self.m = (a * m0 - f(lr) * g).astype(self.f)
            x = (x - a * m0).astype(self.f) + (f(1) + a) * self.m
        elif r == ADAGRAD:
            self.m = (self.m + g * g).astype(self.f)
            x = x - f(lr) * g / (np.sqrt(self.m) + f(eps))
        elif r == RMSPROP:
            self.m = (a * self.m + (f(1) - a) * g * g).astype(self.f)
            x = x - f(lr) * g / (np.sqrt(self.m) + f(eps))
        else:
            self.m = (a * self.m + (f(1) - a) * g).astype(self.f)
            self.v = (b * self.v + (f(1) - b) * g * g).astype(self.f)
            self.t += 1
            step = float(f32(lr)) * np.sqrt(1 - float(f32(beta)) ** self.t) / (1 - float(f32(alpha)) ** self.t)
            x = x - f(step) * (self.m / (np.sqrt(self.v) + f(eps)))
        return x.astype(self.f), norm, count
