// include/QuBLAS_amd.h on its own: the QgemulBatched lowering (batched_probe_common.hpp).
#include "QuBLAS_amd.h"

using namespace QuBLAS_amd;
#include "batched_probe_common.hpp"

int main() { return batched_probe_main(); }
