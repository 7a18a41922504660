// Lowers chains with a complex x complex ThenMul / ThenRmul through include/QuBLAS_amd.h and prints their C-ABI form (no GPU):
// tests/test_cmul_lowering.py compares the bytes with the Python lowering's and with the reference-header binding's
// (ref_binding_cmul_probe.cpp: the same chains, cmul_probe_common.hpp).
#include "QuBLAS_amd.h"
using namespace QuBLAS_amd;
#include "cmul_probe_common.hpp"

int main()
{
    lower_and_print_chains();
    return 0;
}
