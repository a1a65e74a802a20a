"""CriticObs (reference model/common/critic.py:15-54): ResidualMLP([Do*To, h, h, h, 1], Mish) with
residual_style=True (the fine-tune cfgs), or the class default residual_style=False: the plain
MLP([Do*To, h, h, h, 1], Mish). use_layernorm=True with residual_style=True puts Keras' LayerNormalization before
the residual block's two Mish sites (model/common/mlp.py) at hidden width 256. The plain head with layer norm (three
norm sites, Keras' default epsilon) is CriticObsPlainLN below: CriticObs itself keeps refusing
(residual_style=False, use_layernorm=True), the refusal tests/test_critic_plain_cpu.py pins, and names that class.

Construction mirrors the reference kwargs; the forward runs the HIP value kernel
(dppo_critic_forward) once the owning VPGDiffusion has placed the weights on the device."""
import numpy as np
import torch

from .mlp import MLP, ResidualMLP

# the one hidden width the critic row tile instantiates (csrc/rowtile.hip dispatch_critic)
PLAIN_HIDDEN = 256


class CriticObs:
    _plain_layernorm = False   # CriticObsPlainLN: the layer-normed plain head is accepted

    def __init__(self, cond_dim, mlp_dims, activation_type="Mish", use_layernorm=False, residual_style=False,
                 **kwargs):
        if activation_type != "Mish":
            raise NotImplementedError("the critic kernels implement the cfg's Mish activation")
        self.cond_dim = cond_dim
        dims = [cond_dim] + list(mlp_dims) + [1]
        if residual_style:
            self.net = ResidualMLP(dims, activation_type=activation_type, use_layernorm=use_layernorm)
        else:
            shape = f"mlp_dims = [{PLAIN_HIDDEN}, {PLAIN_HIDDEN}, {PLAIN_HIDDEN}] (three equal hidden layers, Mish, no layernorm)"
            if use_layernorm and not self._plain_layernorm:
                raise NotImplementedError(f"CriticObs(residual_style=False, use_layernorm=True): the plain critic kernels implement {shape}"
                                          "; the layer-normed plain head is model.common.critic.CriticObsPlainLN (critic_layernorm=True "
                                          "in ops.ModelDims), the layer-normed residual critic CriticObs(residual_style=True)")
            if list(mlp_dims) != [PLAIN_HIDDEN] * 3:
                raise NotImplementedError(f"CriticObs(residual_style=False, mlp_dims={list(mlp_dims)}): the plain critic "
                                          f"kernels implement {shape}")
            self.net = MLP(dims, activation_type=activation_type, use_layernorm=use_layernorm)
        self.head = "residual" if residual_style else "plain"   # ops.ModelDims.critic_head
        self.use_layernorm = bool(use_layernorm)                # ops.ModelDims.critic_layernorm
        self.hidden = self.net.hidden
        self._owner = None

    def init_params(self, rng):
        return self.net.init_params(rng)

    def __call__(self, cond):
        """cond: {"state": [B, To, Do]} or [B, To*Do] -> values [B, 1] (device tensor)."""
        if self._owner is None:
            raise RuntimeError("CriticObs has no device weights yet (construct it through PPODiffusion)")
        return self._owner.critic_values(cond)[:, None]


class CriticObsPlainLN(CriticObs):
    """The reference's CriticObs(residual_style=False, use_layernorm=True): MLP([Do*To, 256, 256, 256, 1], Mish) with
    Dense -> LayerNormalization (epsilon 1e-3) -> Mish per hidden layer (model/common/mlp.py:62-78). A class of its
    own only because CriticObs's refusal of those two kwargs is pinned by an existing test; it takes CriticObs's
    kwargs, with residual_style and use_layernorm fixed at (False, True), and is a CriticObs in every other respect
    (head "plain", use_layernorm True: cfgs name it as the critic's `_target_`)."""
    _plain_layernorm = True

    def __init__(self, cond_dim, mlp_dims, activation_type="Mish", use_layernorm=True, residual_style=False, **kwargs):
        if residual_style or not use_layernorm:
            raise ValueError("CriticObsPlainLN is the plain head with layer norm: residual_style=False, use_layernorm=True "
                             "(every other combination is CriticObs)")
        super().__init__(cond_dim, mlp_dims, activation_type=activation_type, use_layernorm=True, residual_style=False, **kwargs)
