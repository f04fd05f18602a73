// vs_weights_impl.h — the packed-parameter handle behind `vs_weights` (include/vs_scorer.h): its layout is
// vs_weights_layout.h, its code vs_weights.cpp.  Read by the scoring C ABI (vs_scorer.cpp), the training
// C ABI (vs_train.cpp) and the optimizer (vs_optim.hip).  Internal: not part of the public headers.
#pragma once
#include <stddef.h>

#include "vs_error.h"
#include "vs_forward_plan.h"      // VSW_*: the image families
#include "vs_scorer.h"
#include "vs_weights_layout.h"

struct vs_weights : VsWeightsLayout {
    vs_model_desc desc;
    float *blob = nullptr;        // one device allocation
    int device = 0;               // the device the blob lives on
    int norm_width = 0;           // vs_weights_set_norm_width: true d_model of a model embedded in this (wider) shape; 0 = desc.d_model
    int dn() const { return norm_width > 0 ? norm_width : desc.d_model; }
    bool embedded() const { return norm_width > 0 && norm_width != desc.d_model; }
    const float *p(size_t off) const { return blob + off; }
    // second device allocation (transposed weights + a zero vector): made by the first call that needs a training family, or
    // by vs_train_prepare - never for a scoring-only user
    mutable float *tblob = nullptr;
    const float *tp(size_t off) const { return tblob + off; }

    // Kernel-layout IMAGES of the parameters: built by vsw_ensure() when a call that reads the family runs, never at pack /
    // update time (a training step never pays for the f16x3 / bf16 images, a large-batch scorer never for the fragment-major
    // latency copies).  built[i]: the `version` family 1 << i was built from.
    unsigned long long version = 0;       // bumped by every pack / update / native optimizer step
    mutable unsigned long long built[VSW_NUM_FAMILIES] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};

    // Stream ordering of everything above: the last stream that wrote the parameters or (re)built an image, and an event
    // recorded behind that work.  A call on ANOTHER stream first waits for the event (hipStreamWaitEvent: no host
    // synchronisation), so the host-side version stamps never run ahead of the device.
    mutable void *order_event = nullptr;  // hipEvent_t, created on first use
    mutable void *order_stream = nullptr; // hipStream_t of the recorded work (meaningful only while order_event != nullptr)
    mutable bool order_recorded = false;
};

// (re)builds the image families in `families` that are older than the handle's parameters, stream-ordered on `stream`, after
// waiting (on the device) for whatever another stream last did to the handle.
// A handle's calls must be issued on ONE stream at a time (or be ordered by the caller): include/vs_scorer.h.
int vsw_ensure(const vs_weights *w, unsigned families, void *stream);
// stream ordering helpers: vsw_mark() after parameter writes / image rebuilds were enqueued on `stream`; vsw_order() before a
// call on `stream` reads them (a no-op when it is the same stream)
void vsw_mark(const vs_weights *w, void *stream);
void vsw_order(const vs_weights *w, void *stream);
