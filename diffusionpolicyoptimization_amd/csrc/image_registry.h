// image_registry.h — what the library remembers about a packed image, keyed by the image's address: the
// attributes its last pack recorded (ImageAttrs) and, for an actor image an optimizer step left without its
// split-sampler tables, the record the sampler's refresh re-derives them from. HIP-free.
//
// The rule: only an extern "C" entry (or the one launcher it calls) reads this table, once, and passes
// NetSpecs down by value. Packing entries commit after a pack that returned DPPO_OK; nothing else changes attributes.
#pragma once
#include "dppo_layout.h"

// the actor image's split-sampler tables are stale (packed without them by a step that deferred them); temb:
// the TEMB table is stale too
struct StaleTables { NetSpec net; const float* params; bool temb; };
constexpr int DPPO_MAX_STALE = 32;   // images with a pending refresh at one time

// defaults (ReLU / RESIDUAL / LN_OFF) for an address no pack recorded
ImageAttrs dppo_image_attrs(const void* packed);
// all-default attributes on an image with no pending refresh erase its entry
void dppo_image_commit(const void* packed, ImageAttrs attrs);
// the latest mark of an image replaces its record; false: DPPO_MAX_STALE other images are pending (nothing changes)
bool dppo_image_mark_stale(const void* packed, const StaleTables& rec);
// the pending record, removed from the table (the attributes stay); false: none
bool dppo_image_take_stale(const void* packed, StaleTables* rec);
void dppo_image_clear_stale(const void* packed);
// the image's memory is being released: its address reads as never packed from here on
void dppo_image_forget(const void* packed);

// A schedule table's attributes, keyed by the table's device address like an image's (include/dppo.h, the schedule
// table): the clip bound of x_recon (+inf: none) and whether the network predicts x0 instead of epsilon. The same
// rule: an extern "C" entry reads the record once and passes it down by value.
struct SchedParams { float clip = 1.f; int predict_x0 = 0; };
// defaults ({1.0, epsilon}) for an address nobody recorded
SchedParams dppo_sched_params(const void* sched);
// all-default parameters erase the entry
void dppo_sched_commit(const void* sched, SchedParams p);
// the table's memory is being released: its address reads as never recorded from here on
void dppo_sched_forget(const void* sched);
