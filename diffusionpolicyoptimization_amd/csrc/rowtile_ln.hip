// rowtile_ln.hip — the critic row tile's LN axis (a layer-normed critic image, include/dppo.h
// dppo_pack_critic_ln): the instantiations of critic_rowtile_body<..., LN = true> (rowtile_critic.cuh) for both
// heads, both modes and the three precisions, 32 rows on 8 waves like the tiles without the norm. They run the
// plain 8-wave kernel entry: the TRAIN tiles take 223-253 registers, so there is no 128-register _o4 form.
#include "rowtile_critic.cuh"

template <class P, int HEAD>
static int dispatch_critic_ln(const CriticArgs& a, hipStream_t s, bool dry) {
    constexpr int MT = 2, WAVES = 8;   // rowtile.hip CRITIC_MT and its wave count
    if (a.HC / (16 * WAVES) != 2) return dppo_set_error(DPPO_EUNSUPPORTED, "critic: hidden %d not instantiated", a.HC);
    return a.mode == ROWS_TRAIN ? launch_critic_t<P, MT, 2, true, WAVES, false, HEAD, true>(a, s, dry)
                                : launch_critic_t<P, MT, 2, false, WAVES, false, HEAD, true>(a, s, dry);
}
template <class P>
static int dispatch_critic_ln_head(const CriticArgs& a, bool plain, hipStream_t s, bool dry) {
    return plain ? dispatch_critic_ln<P, DPPO_HEAD_PLAIN>(a, s, dry) : dispatch_critic_ln<P, DPPO_HEAD_RESIDUAL>(a, s, dry);
}

// dppo_ppo_plan's field for the critic's row tile, which that query (six outputs, no image) does not have: host
// arithmetic only. Both forms run 32 rows on 8 waves (rowtile.hip CRITIC_MT, launch_critic_rowtile); the tiles without
// layer norm run the 128-register entry (two tiles per CU), the layer-normed ones the uncapped entry above
extern "C" int dppo_ppo_plan_critic(const dppo_dims* d, int precision, int critic_head, int critic_layernorm, int* out) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(dppo_head_ok(critic_head), "dppo_ppo_plan_critic: bad head %d (DPPO_HEAD_RESIDUAL or DPPO_HEAD_PLAIN)", critic_head);
    DPPO_CHECK(dppo_ln_ok(critic_layernorm), "dppo_ppo_plan_critic: bad layernorm %d (DPPO_LN_OFF or DPPO_LN_ON)", critic_layernorm);
    DPPO_CHECK(out, "dppo_ppo_plan_critic: out is NULL");
    out[0] = 32;
    out[1] = 8;
    out[2] = critic_layernorm == DPPO_LN_ON ? 0 : 1;
    return DPPO_OK;
}

int launch_critic_rowtile_ln(const CriticArgs& a, const NetSpec& net, hipStream_t s, bool dry) {
    return net.precision == DPPO_BF16 ? dispatch_critic_ln_head<PolicyBF16>(a, net.plain(), s, dry)
         : net.precision == DPPO_F16  ? dispatch_critic_ln_head<PolicyF16>(a, net.plain(), s, dry)
                                      : dispatch_critic_ln_head<PolicyF32>(a, net.plain(), s, dry);
}
