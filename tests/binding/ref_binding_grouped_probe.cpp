// The lowerings of amd_header_grouped_probe.cpp on the REFERENCE header's own types through include/qgemul_reference_binding.hpp;
// compiled by tests/test_grouped_binding.py where the reference header is present.
#include "QuBLAS.h"
#include "qgemul_reference_binding.hpp"
using namespace QuBLAS;
#include "grouped_probe_common.hpp"

int main() { return grouped_probe_main(); }
