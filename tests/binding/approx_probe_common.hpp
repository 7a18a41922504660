// shared by the two ThenApprox lowering probes (tests/test_approx_plan.py): the chain's C-ABI form as hex bytes, one JSON line
#pragma once
#include <array>
#include <cstdio>

#include "qgemul.h"

template <class T>
static void hex_bytes(const T& v)
{
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    std::printf("\"");
    for (size_t i = 0; i < sizeof(T); ++i) std::printf("%02x", p[i]);
    std::printf("\"");
}

static void print_chain(const char* name, const qgemul_epilogue& ep, const std::array<const qgemul_approx*, QG_MAX_EW>& ax)
{
    std::printf("{\"name\":\"%s\",\"ep\":", name);
    hex_bytes(ep);
    std::printf(",\"ax\":[");
    for (int k = 0; k < QG_MAX_EW; ++k) {
        if (k) std::printf(",");
        if (ax[k]) hex_bytes(*ax[k]);
        else std::printf("null");
    }
    std::printf("]}\n");
}
