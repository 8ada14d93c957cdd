"""`tensorflow_probability.python.distributions` as far as Optimizers/optimizer_cem_gmm_tf.py uses it:

    MixtureSameFamily(mixture_distribution=Categorical(probs=[p, 1 - p]), components_distribution=Normal(loc, scale))
    .sample(sample_shape=[N]), .components_distribution.mean() / .stddev(), .mixture_distribution, Distribution (annotation)

Written for tests/golden/make_golden_gmm.py; not TensorFlow Probability source.  Semantics after TFP's documentation:
Normal(loc, scale) with loc / scale [H,C,2] has batch shape [H,C,2]; Categorical(probs=[2]) has a SCALAR batch shape, so
MixtureSameFamily takes the last batch axis of the components as the component axis and `sample([N])` draws ONE component index
per sample: the whole [H,C] plan of a rollout comes from one component.

Draw convention of `sample([N])` (the one include/ctk_hip.h documents for ctk_step): N*H*C standard normals, row-major [N,H,C],
then N uniforms in [0,1); sample n takes component 0 iff uniform[n] < probs[0]; value = loc_k + z * scale_k.  The bit stream is
torch's (seeded with `seed()`), not TFP's; every call's raw draws are appended to DRAW_LOG as (normals, uniforms)."""
import numpy as _np
import torch as _torch

_GEN = _torch.Generator().manual_seed(0)
DRAW_LOG = []


def seed(value):
    _GEN.manual_seed(int(value))
    DRAW_LOG.clear()


def _t(x):
    if isinstance(x, (list, tuple)):
        return _torch.stack([_t(v) for v in x])
    return x.to(_torch.float32) if isinstance(x, _torch.Tensor) else _torch.as_tensor(_np.asarray(x, _np.float32))


class Distribution:
    pass


class Normal(Distribution):
    def __init__(self, loc, scale):
        self.loc, self.scale = _t(loc), _t(scale)

    def mean(self):
        return self.loc

    def stddev(self):
        return self.scale


class Categorical(Distribution):
    def __init__(self, probs):
        self.probs = _t(probs)
        assert self.probs.ndim == 1


class MixtureSameFamily(Distribution):
    def __init__(self, mixture_distribution, components_distribution):
        assert mixture_distribution.probs.shape[0] == 2 and components_distribution.loc.shape[-1] == 2
        self.mixture_distribution = mixture_distribution
        self.components_distribution = components_distribution

    def sample(self, sample_shape):
        n, = (int(v) for v in sample_shape)
        loc, scale = self.components_distribution.loc, self.components_distribution.scale
        event = tuple(loc.shape[:-1])
        z = _torch.normal(mean=0.0, std=1.0, size=(n,) + event, generator=_GEN, dtype=_torch.float32)
        u = _torch.rand(n, generator=_GEN, dtype=_torch.float32)
        DRAW_LOG.append((z.numpy().copy(), u.numpy().copy()))
        k = _torch.where(u < self.mixture_distribution.probs[0], 0, 1)
        loc_k = _torch.movedim(loc, -1, 0)[k]
        scale_k = _torch.movedim(scale, -1, 0)[k]
        return loc_k + z * scale_k
