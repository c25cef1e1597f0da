"""The four device calls of bias.correct on CPU tensors, from the restatement: a stand-in `ops` for the host tests."""
import numpy as np
import torch

from tests import prep_bias_ref as R


class BiasMixin:
    def prep_bias_log(self, v, mask="nonzero"):
        u, m = R.log_mask(v.numpy())
        return torch.from_numpy(u), torch.from_numpy(m.astype(np.uint8))

    def prep_bias_hist(self, u, m, f, stride, offset):
        grid = np.ix_(*[np.arange(o, n, s) for n, s, o in zip(u.shape, stride, offset)])
        r = (u.numpy()[grid] - f.numpy())[m.numpy()[grid] != 0]
        if r.size == 0:
            return np.zeros(R.BINS, dtype=np.int64), 0.0, 0.0, 0
        return R.histogram(r) + (int(r.size),)

    def prep_bias_fit(self, u, m, f, stride, offset, level, lo, hi, table, phi, lattice_):
        idx = [np.arange(o, n, s) for n, s, o in zip(u.shape, stride, offset)]
        axes = [R.dense_weights(n, level, i) for n, i in zip(u.shape, idx)]
        grid = np.ix_(*idx)
        _, p, df, s1, s2 = R.fit_step(u.numpy()[grid], f.numpy(), m.numpy()[grid] != 0, np.asarray(table), lo, hi, axes)
        phi.copy_(torch.from_numpy(p.reshape(-1)))
        lattice_ += phi
        f += torch.from_numpy(df.astype(np.float32))
        return float(s1), float(s2)

    def prep_bias_apply(self, v, m, lattices):
        x, at, field = v.numpy(), 0, 0.0
        for level in range(R.LEVELS):
            p = 2 ** level + 3
            field = field + R.evaluate(lattices.numpy()[at:at + p ** 3].reshape(p, p, p),
                                     [R.dense_weights(n, level, np.arange(n)) for n in x.shape])
            at += p ** 3
        e = np.exp(field)
        inside = e[m.numpy() != 0].astype(np.float32)
        with np.errstate(invalid="ignore"):
            return torch.from_numpy((x.astype(np.float64) / e).astype(np.float32)), float(inside.min()), float(inside.max())
