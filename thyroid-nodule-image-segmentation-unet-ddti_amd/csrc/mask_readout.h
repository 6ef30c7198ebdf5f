// The mask readout of unet_mask_counts (utils/trainer.py:217-220), the one definition every
// feature reads its masks through (surf.h includes it for the device and the host; a header built
// for the host alone, such as export.h under EXPORT_HOST_ONLY, includes it without any HIP header).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef READOUT_HD
#define READOUT_HD inline
#endif

// sigmoid(x) > 0.5 in float32, as torch forms it
READOUT_HD bool surf_pred(float x) { return 1.f / (1.f + expf(-x)) > 0.5f; }
// numpy astype(uint8) truncation of the {0, 1} float targets; == 1 is foreground
READOUT_HD uint8_t surf_target_u8(float t) { return (uint8_t)(int)t; }
READOUT_HD bool surf_target(float t) { return surf_target_u8(t) == 1; }
