// Interpolation level 2 as its own translation unit (runtime.hipcc_commands; see lfsd_cubic.inc).
#include "lfsd_internal.h"
#include "lfsd_cubic.inc"
