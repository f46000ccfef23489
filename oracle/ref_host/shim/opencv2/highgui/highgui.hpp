// Empty on purpose: the host build of the stage headers needs nothing from this library (see ../ref_shim.h).
#include "ref_shim.h"
