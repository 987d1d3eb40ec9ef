// K1 + IPC reductions instantiated for F8E4M3 (see reduce_impl.h)
#include "reduce_impl.h"

PDCC_REDUCE_DTYPE(F8E4M3, PDCC_OPS_FLOAT)
