// y7t_dhn.h -- what the tracker's translation unit needs of the Deep Hungarian Net object (csrc/y7t_dhn.hip): where a frame's distance matrix and the
// network's output live inside the object, and the forward as a sequence of launches without a host round trip.
#pragma once
#include "y7t_common.h"

// supported sizes: any h, w >= 1 with h * w <= Y7T_DHN_MAX_T (the epochs of the hand-off are 32-bit: 4 passes x T steps + 1)
#define Y7T_DHN_MAX_T (1 << 20)

struct Y7TDhnView {
    int max_h, max_w;      // what y7t_dhn_init sized the workspace for: any h x w with h * w <= max_h * max_w runs
    float* D;              // [max_h * max_w]  a frame's distance matrix (the tracker's front program writes it)
    float* out;            // [max_h * max_w]  the network's sigmoid output for it
    int* hw;               // [4]              rows, columns of the frame's matrix (device; the front program writes them)
    unsigned* status;      // the forward's status word: non-zero after a bounded spin gave up
};

// the object at `dhn` as y7t_dhn_init noted it (host side) -> 0, or Y7T_E_STATE for an address that was never initialised
int y7t_dhn_view(const void* dhn, Y7TDhnView* v);
// enqueue the forward of D (h x w, device) -> out (h x w, device); no synchronisation, the status word is left on the device
int y7t_dhn_enqueue(void* dhn, const float* D, int h, int w, float* out, hipStream_t stream);
