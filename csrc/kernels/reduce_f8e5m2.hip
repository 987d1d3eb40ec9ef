// K1 + IPC reductions instantiated for F8E5M2 (see reduce_impl.h)
#include "reduce_impl.h"

PDCC_REDUCE_DTYPE(F8E5M2, PDCC_OPS_FLOAT)
