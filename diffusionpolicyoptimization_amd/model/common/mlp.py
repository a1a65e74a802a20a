"""Residual MLP parameter containers (reference model/common/mlp.py:95-206).

On MI355X the MLP has no per-layer Python objects: its weights are one flat fp32 buffer in the
Keras layout (include/dppo.h) that the HIP kernels consume through a packed fragment image. These
classes hold the configuration, validate it against what the kernels implement, and create the
seeded Keras-style initialisation (glorot_uniform kernels, zero biases)."""
import math

import numpy as np

# the actor's activations (include/dppo.h DPPO_ACT_*; GELU is the erf form). The critic's shapes below require Mish
# themselves (_critic_ln_shape, MLP.layers4; CriticObs refuses every other name before it gets here)
SUPPORTED_ACTIVATIONS = ("ReLU", "Mish", "ELU", "GELU", "Softplus")
# layer normalisation is implemented for the critic's shape only: [in, 256, 256, 256, 1] with Mish, the one hidden
# width the critic row tile instantiates (csrc/rowtile.hip; include/dppo.h dppo_pack_critic_ln)
LAYERNORM_HIDDEN = 256


def _critic_ln_shape(dim_list, activation_type):
    return (len(dim_list) == 5 and dim_list[1] == dim_list[2] == dim_list[3] == LAYERNORM_HIDDEN and dim_list[4] == 1
            and activation_type == "Mish")


def _ln_params(h, sites, prefix):
    """Keras' LayerNormalization variables: gamma ones, beta zeros (ln{k}_g, ln{k}_b after out_b in the flat layout)."""
    p = {}
    for k in range(1, sites + 1):
        p[f"{prefix}ln{k}_g"] = np.ones(h, np.float32)
        p[f"{prefix}ln{k}_b"] = np.zeros(h, np.float32)
    return p


def glorot_uniform(rng, fan_in, fan_out):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


class ResidualMLP:
    """dims [in, h, h, h, out]: in-Dense, ONE pre-activation two-Dense block (mlp.py:121-129), out-Dense.
    use_layernorm (the critic's shape [in, 256, 256, 256, 1] with Mish only): the block's two pre-activation
    LayerNormalizations, epsilon 1e-6 (mlp.py:174-176, 190-202):
        h1 = in(x);  u1 = mish(LN_1(h1));  h2 = l1(u1);  u2 = mish(LN_2(h2));  h3 = l2(u2) + h1;  y = out(h3)"""

    def __init__(self, dim_list, activation_type="Mish", out_activation_type="Identity", use_layernorm=False,
                 use_layernorm_final=False, dropout=0):
        dim_list = list(dim_list)
        if len(dim_list) != 5 or not (dim_list[1] == dim_list[2] == dim_list[3]):
            raise NotImplementedError(f"ResidualMLP {dim_list}: the kernels implement [in, h, h, h, out] "
                                      "(one residual block), the shape every fine-tune cfg uses")
        if use_layernorm_final or dropout or (use_layernorm and not _critic_ln_shape(dim_list, activation_type)):
            raise NotImplementedError("layernorm/dropout are not used by the fine-tune cfgs and not implemented (use_layernorm: "
                                      f"for the critic's [in, {LAYERNORM_HIDDEN}, {LAYERNORM_HIDDEN}, {LAYERNORM_HIDDEN}, 1] with Mish only)")
        if out_activation_type != "Identity":
            raise NotImplementedError("out_activation_type must be Identity")
        self.use_layernorm = bool(use_layernorm)
        if activation_type not in SUPPORTED_ACTIVATIONS:
            raise NotImplementedError(f"activation {activation_type} not implemented (the kernels implement {', '.join(SUPPORTED_ACTIVATIONS)})")
        self.dim_list = dim_list
        self.activation_type = activation_type

    @property
    def hidden(self):
        return self.dim_list[1]

    def init_params(self, rng, prefix=""):
        i, h, o = self.dim_list[0], self.dim_list[1], self.dim_list[-1]
        return {prefix + "in_w": glorot_uniform(rng, i, h), prefix + "in_b": np.zeros(h, np.float32),
                prefix + "l1_w": glorot_uniform(rng, h, h), prefix + "l1_b": np.zeros(h, np.float32),
                prefix + "l2_w": glorot_uniform(rng, h, h), prefix + "l2_b": np.zeros(h, np.float32),
                prefix + "out_w": glorot_uniform(rng, h, o), prefix + "out_b": np.zeros(o, np.float32),
                **_ln_params(h, 2 if self.use_layernorm else 0, prefix)}


class MLP:
    """Plain MLP (mlp.py:35-92), reached from cfgs with residual_style: False. The kernels implement the
    two-hidden-layer shape of the reference's default mlp_dims, dims [in, h, h, out]:
        h1 = in(x);  u1 = act(h1);  h2 = l1(u1);  a = act(h2);  y = out(a)
    (the residual network with the l2 layer and the skip removed; include/dppo.h DPPO_HEAD_PLAIN). For the critic
    (CriticObs residual_style=False) they also implement three equal hidden layers with one output and Mish,
    dims [in, h, h, h, 1]:
        h1 = in(x);  u1 = mish(h1);  h2 = l1(u1);  u2 = mish(h2);  h3 = l2(u2);  u3 = mish(h3);  y = out(u3)
    (include/dppo.h dppo_pack_critic_head). With use_layernorm that critic shape (hidden 256) is Dense ->
    LayerNormalization (Keras' default epsilon 1e-3) -> Mish per hidden layer (mlp.py:62-78), no norm on the output
    layer: u_k = mish(LN_k(h_k)) (dppo_pack_critic_ln). Every other shape or option is a loud error rather than a
    silent fallback."""

    SHAPE = "[in, h, h, out] with out_activation_type='Identity' and no layernorm, dropout or append"
    CRITIC_SHAPE = "[in, h, h, h, 1] with Mish, out_activation_type='Identity' and no layernorm, dropout or append"

    def __init__(self, dim_list, append_dim=0, append_layers=None, activation_type="Tanh", out_activation_type="Identity",
                 use_layernorm=False, use_layernorm_final=False, dropout=0):
        dim_list = list(dim_list)
        # the critic's shape: four Dense layers (in, l1, l2, out), the flat layout of the residual critic
        self.layers4 = (len(dim_list) == 5 and dim_list[1] == dim_list[2] == dim_list[3] and dim_list[4] == 1
                        and activation_type == "Mish")
        if not self.layers4 and (len(dim_list) != 4 or dim_list[1] != dim_list[2]):
            raise NotImplementedError(f"MLP {dim_list}: the kernels implement the plain head {self.SHAPE} "
                                      f"(the critic's: {self.CRITIC_SHAPE})")
        if use_layernorm and self.layers4 and not _critic_ln_shape(dim_list, activation_type):
            raise NotImplementedError(f"MLP {dim_list} with use_layernorm: the layer-normed critic kernels implement hidden width "
                                      f"{LAYERNORM_HIDDEN}")
        if (use_layernorm and not self.layers4) or use_layernorm_final or dropout or append_dim or append_layers:
            raise NotImplementedError(f"MLP layernorm / dropout / append: the kernels implement the plain head {self.SHAPE}")
        if out_activation_type != "Identity":
            raise NotImplementedError(f"MLP out_activation_type {out_activation_type!r}: the kernels implement {self.SHAPE}")
        if activation_type not in SUPPORTED_ACTIVATIONS:
            raise NotImplementedError(f"activation {activation_type} not implemented (the kernels implement {', '.join(SUPPORTED_ACTIVATIONS)})")
        self.dim_list = dim_list
        self.activation_type = activation_type
        self.use_layernorm = bool(use_layernorm)

    @property
    def hidden(self):
        return self.dim_list[1]

    def init_params(self, rng, prefix=""):
        """in, l1 and out only: a plain head has no l2 (its range of the flat layout stays zero). The critic's
        [in, h, h, h, 1] has l2 as its third Dense layer, so all four."""
        i, h, o = self.dim_list[0], self.dim_list[1], self.dim_list[-1]
        p = {prefix + "in_w": glorot_uniform(rng, i, h), prefix + "in_b": np.zeros(h, np.float32),
             prefix + "l1_w": glorot_uniform(rng, h, h), prefix + "l1_b": np.zeros(h, np.float32)}
        if self.layers4:
            p.update({prefix + "l2_w": glorot_uniform(rng, h, h), prefix + "l2_b": np.zeros(h, np.float32)})
        p.update({prefix + "out_w": glorot_uniform(rng, h, o), prefix + "out_b": np.zeros(o, np.float32)})
        p.update(_ln_params(h, 3 if self.use_layernorm else 0, prefix))
        return p
