// image_registry.cpp — the one address-keyed table of libdppo_hip.so (image_registry.h).
#include "image_registry.h"
#include <mutex>
#include <vector>

namespace {
struct Entry { const void* packed; ImageAttrs attrs; bool stale; StaleTables rec; };
std::mutex g_mu;
std::vector<Entry> g_images;
struct SchedEntry { const void* sched; SchedParams p; };
std::vector<SchedEntry> g_scheds;   // only tables whose parameters are not the defaults

Entry* find(const void* packed) {
    for (Entry& e : g_images)
        if (e.packed == packed) return &e;
    return nullptr;
}
// only images with something to remember are listed
void drop_if_default(Entry* e) {
    const ImageAttrs& a = e->attrs;
    if (e->stale || a.act != DPPO_ACT_RELU || a.head != DPPO_HEAD_RESIDUAL || a.ln != DPPO_LN_OFF) return;
    *e = g_images.back();
    g_images.pop_back();
}
}  // namespace

ImageAttrs dppo_image_attrs(const void* packed) {
    std::lock_guard<std::mutex> lk(g_mu);
    const Entry* e = find(packed);
    return e ? e->attrs : ImageAttrs();
}

void dppo_image_commit(const void* packed, ImageAttrs attrs) {
    std::lock_guard<std::mutex> lk(g_mu);
    Entry* e = find(packed);
    if (!e) {
        g_images.push_back(Entry{packed, attrs, false, StaleTables{}});
        e = &g_images.back();
    }
    e->attrs = attrs;
    drop_if_default(e);
}

bool dppo_image_mark_stale(const void* packed, const StaleTables& rec) {
    std::lock_guard<std::mutex> lk(g_mu);
    Entry* e = find(packed);
    if (!e || !e->stale) {
        int pending = 0;
        for (const Entry& x : g_images) pending += x.stale ? 1 : 0;
        if (pending >= DPPO_MAX_STALE) return false;
    }
    if (!e) {
        g_images.push_back(Entry{packed, ImageAttrs(), false, StaleTables{}});
        e = &g_images.back();
    }
    e->stale = true;
    e->rec = rec;
    return true;
}

bool dppo_image_take_stale(const void* packed, StaleTables* rec) {
    std::lock_guard<std::mutex> lk(g_mu);
    Entry* e = find(packed);
    if (!e || !e->stale) return false;
    *rec = e->rec;
    e->stale = false;
    drop_if_default(e);
    return true;
}

void dppo_image_clear_stale(const void* packed) {
    StaleTables unused;
    dppo_image_take_stale(packed, &unused);
}

void dppo_image_forget(const void* packed) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (Entry* e = find(packed)) {
        *e = g_images.back();
        g_images.pop_back();
    }
}

SchedParams dppo_sched_params(const void* sched) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (const SchedEntry& e : g_scheds)
        if (e.sched == sched) return e.p;
    return SchedParams();
}

namespace {
void sched_erase_locked(const void* sched) {
    for (SchedEntry& e : g_scheds)
        if (e.sched == sched) {
            e = g_scheds.back();
            g_scheds.pop_back();
            return;
        }
}
}  // namespace

void dppo_sched_forget(const void* sched) {
    std::lock_guard<std::mutex> lk(g_mu);
    sched_erase_locked(sched);
}

void dppo_sched_commit(const void* sched, SchedParams p) {
    std::lock_guard<std::mutex> lk(g_mu);   // one critical section: no reader sees the defaults in between
    sched_erase_locked(sched);
    if (p.clip == 1.f && !p.predict_x0) return;
    g_scheds.push_back(SchedEntry{sched, p});
}
