// Stub (ours): forwards to ref_shim.h, see there.
#include "ref_shim.h"
