// The class-plane variants of score_kernel, in a translation unit of their own because of one compiler flag.  The source —
// kernel, launcher and the flag itself with its reason — is in nmscan_device.h ("the scoring kernel").
#define NM_SCORE_KERNEL_SOURCE
#define NM_SCORE_CLASSES_UNIT
#include "nmscan_device.h"
