// Stand-alone check of csrc/image_registry.cpp and of the layouts' layer-norm tail (csrc/dppo_layout.h), built
// with -fsanitize=address,undefined by tests/test_image_registry_cpu.py. Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "image_registry.h"

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static bool is_default(ImageAttrs a) { return a.act == DPPO_ACT_RELU && a.head == DPPO_HEAD_RESIDUAL && a.ln == DPPO_LN_OFF; }
static bool same(ImageAttrs a, ImageAttrs b) { return a.act == b.act && a.head == b.head && a.ln == b.ln; }

// hopper (tests/helpers.py HOPPER)
static Dims hopper() {
    Dims D = {};
    D.Do = 11; D.Da = 3; D.Ta = 4; D.To = 1; D.TD = 16; D.H = 512; D.HC = 256; D.K = 20; D.KF = 10; D.TS = 1;
    D.XD = D.Ta * D.Da; D.SD = D.To * D.Do; D.IN = D.XD + D.TD + D.SD;
    return D;
}

static void registry() {
    static char mem[64];   // addresses only: the registry never dereferences them
    const void* img = mem;
    const ImageAttrs mish_plain{DPPO_ACT_MISH, DPPO_HEAD_PLAIN, DPPO_LN_OFF}, ln{DPPO_ACT_RELU, DPPO_HEAD_RESIDUAL, DPPO_LN_ON};
    StaleTables rec = {actor_net(hopper(), DPPO_BF16, mish_plain), (const float*)(mem + 8), true}, got = {};

    CHECK(is_default(dppo_image_attrs(img)));                 // an unknown address reads defaults
    CHECK(!dppo_image_take_stale(img, &got));
    dppo_image_commit(img, mish_plain);                        // a non-default commit is read back
    CHECK(same(dppo_image_attrs(img), mish_plain));
    CHECK(is_default(dppo_image_attrs(mem + 1)));
    dppo_image_commit(img, ImageAttrs());                      // committing defaults erases the entry
    CHECK(is_default(dppo_image_attrs(img)));

    CHECK(dppo_image_mark_stale(img, rec));                    // a stale mark survives a commit of the same address
    dppo_image_commit(img, ln);
    dppo_image_commit(img, ImageAttrs());
    CHECK(dppo_image_take_stale(img, &got));
    CHECK(got.params == rec.params && got.temb && got.net.hidden == 512 && got.net.precision == DPPO_BF16 &&
          got.net.act == DPPO_ACT_MISH && got.net.head == DPPO_HEAD_PLAIN && got.net.temb_steps == 20);
    CHECK(!dppo_image_take_stale(img, &got));                  // taken once
    dppo_image_commit(img, ln);
    CHECK(dppo_image_mark_stale(img, rec));
    CHECK(dppo_image_take_stale(img, &got));                   // take_stale removes only the record
    CHECK(same(dppo_image_attrs(img), ln));
    CHECK(dppo_image_mark_stale(img, rec));
    dppo_image_clear_stale(img);
    CHECK(!dppo_image_take_stale(img, &got) && same(dppo_image_attrs(img), ln));

    CHECK(dppo_image_mark_stale(img, rec));                    // forget clears both
    dppo_image_forget(img);
    CHECK(is_default(dppo_image_attrs(img)) && !dppo_image_take_stale(img, &got));
    dppo_image_forget(img);                                    // and an unknown address is a no-op
    dppo_image_commit(img, ImageAttrs{DPPO_ACT_MISH, DPPO_HEAD_RESIDUAL, DPPO_LN_OFF});   // a new commit starts from defaults
    CHECK(dppo_image_attrs(img).act == DPPO_ACT_MISH && dppo_image_attrs(img).head == DPPO_HEAD_RESIDUAL &&
          dppo_image_attrs(img).ln == DPPO_LN_OFF && !dppo_image_take_stale(img, &got));
    dppo_image_forget(img);

    // the 33rd stale image is refused and the first 32 are intact
    static char many[DPPO_MAX_STALE + 1];
    for (int i = 0; i < DPPO_MAX_STALE; ++i) {
        rec.net.time_stride = i + 1;
        CHECK(dppo_image_mark_stale(many + i, rec));
    }
    CHECK(!dppo_image_mark_stale(many + DPPO_MAX_STALE, rec));
    CHECK(is_default(dppo_image_attrs(many + DPPO_MAX_STALE)) && !dppo_image_take_stale(many + DPPO_MAX_STALE, &got));
    rec.net.time_stride = 100;
    CHECK(dppo_image_mark_stale(many + 3, rec));               // re-marking a pending image is no new one
    for (int i = 0; i < DPPO_MAX_STALE; ++i) {
        CHECK(dppo_image_take_stale(many + i, &got));
        CHECK(got.net.time_stride == (i == 3 ? 100 : i + 1));
    }
    CHECK(dppo_image_mark_stale(many + DPPO_MAX_STALE, rec));  // room again
    dppo_image_forget(many + DPPO_MAX_STALE);
}

static void layouts() {
    const Dims D = hopper();
    for (int precision : {DPPO_F32, DPPO_BF16, DPPO_F16})
        for (int act : {DPPO_ACT_RELU, DPPO_ACT_MISH})
            for (int head : {DPPO_HEAD_RESIDUAL, DPPO_HEAD_PLAIN})
                for (int ln : {DPPO_LN_OFF, DPPO_LN_ON}) {
                    const ImageAttrs at{act, head, ln};
                    const NetSpec a = actor_net(D, precision, at), c = critic_net(D, precision, at);
                    const int sites = ln == DPPO_LN_ON ? (head == DPPO_HEAD_PLAIN ? 3 : 2) : 0;
                    CHECK(a.actor() && !c.actor() && a.ln_sites() == 0 && c.ln_sites() == sites);
                    CHECK(c.temb_steps == 0 && c.time_stride == 1 && a.temb_steps == D.K && a.time_stride == D.TS);
                    const NetLayout LA = make_mlp_layout(a), LC = make_mlp_layout(c);
                    const NetOffsets FA = make_flat_offsets(a), FC = make_flat_offsets(c);
                    CHECK(LA.ln_off == LA.total && LC.ln_off == LC.total && FA.ln == FA.count && FC.ln == FC.count);
                    CHECK(LA.image_bytes == LA.total && FA.count_all == FA.count);   // an actor has no tail
                    CHECK(LC.image_bytes - LC.total == (size_t)4 * 2 * sites * D.HC);   // a multiple of 256 B at HC % 128 == 0
                    CHECK(FC.count_all - FC.count == (size_t)2 * sites * D.HC);
                    CHECK(LC.total % 256 == 0 && LC.image_bytes % 256 == 0);
                    // the attributes move nothing before the tail
                    const NetLayout L0 = make_mlp_layout(critic_net(D, precision));
                    CHECK(L0.total == LC.total && L0.off[SEG_T_L1] == LC.off[SEG_T_L1]);
                    CHECK(make_flat_offsets(critic_net(D)).count == FC.count && FC.count == (size_t)134913);
                    CHECK(FA.count == (size_t)553020);
                }
}

int main() {
    registry();
    layouts();
    std::printf(g_failed ? "%d check(s) failed\n" : "image registry and layouts: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
