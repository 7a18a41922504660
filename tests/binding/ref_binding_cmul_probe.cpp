// The chains of amd_header_cmul_probe.cpp on the REFERENCE header's own types through include/qgemul_reference_binding.hpp;
// compiled by tests/test_cmul_lowering.py where the reference header is present.
#include "QuBLAS.h"
#include "qgemul_reference_binding.hpp"
using namespace QuBLAS;
#include "cmul_probe_common.hpp"

int main()
{
    lower_and_print_chains();
    return 0;
}
