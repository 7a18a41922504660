// The lowerings of amd_header_batched_probe.cpp on the REFERENCE header's own types through include/qgemul_reference_binding.hpp;
// compiled by tests/test_batched_plan.py where the reference header is present.
#include "QuBLAS.h"
#include "qgemul_reference_binding.hpp"
using namespace QuBLAS;
#include "batched_probe_common.hpp"

int main() { return batched_probe_main(); }
