// QgemulGrouped_lower of include/QuBLAS_amd.h against Qgemul_lower of each triple (no GPU, no library call: lowering only);
// compiled by tests/test_grouped_binding.py.
#include "QuBLAS_amd.h"
using namespace QuBLAS_amd;
#include "grouped_probe_common.hpp"

int main() { return grouped_probe_main(); }
