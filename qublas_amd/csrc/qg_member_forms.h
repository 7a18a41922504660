// qg_member_forms.h — the geometries of the member kernels, once: the block-diagonal forms of a batched plan (k_mfma_bd, qg_mfma.hip;
// k_mfma_ep_bd, qg_mfma_ep_bd.hip) and the grouped forms (k_mfma_grp, qg_mfma_grp.hip; k_mfma_ep_grp, qg_mfma_ep_grp.hip) are the
// lock-step body (qg_mfma_body.h) on 64 x 64 tiles, 4 waves with one 32 x 32 MFMA tile each, three LDS stages: 1 x 1 limbs on
// 128-byte k-tiles (QG_MFMA_64_BK128), every other limb pair up to 3 x 3 on 64-byte ones (QG_MFMA_LIMB_64).  Each launcher keeps its
// kernel and its own check of the arguments; the table and the pair rule are what they share.
#pragma once
#include "qg_kernels.h"

// SA, SB: limb planes STORED per operand (k_mfma)
template <int LA_, int LB_, int BK_, int SA_ = LA_, int SB_ = LB_>
struct QMemberForm {
    enum { LA = LA_, LB = LB_, BK = BK_, WGM = 2, WGN = 2, TI = 1, TJ = 1, NSTAGE = 3, SA = SA_, SB = SB_ };
    enum { TM = WGM * TI * 32, TN = WGN * TJ * 32, THREADS = 64 * WGM * WGN, LDS = NSTAGE * (LA * TM + LB * TN) * BK };
};

// f(QMemberForm<...>{}) for the form of LA x LB limbs in `variant`; anything else is hipErrorInvalidValue
template <class F>
hipError_t qg_member_form(int LA, int LB, int variant, F&& f)
{
    if (LA == 1 && LB == 1) return variant == QG_MFMA_64_BK128 ? f(QMemberForm<1, 1, 128>{}) : hipErrorInvalidValue;
    if (variant != QG_MFMA_LIMB_64) return hipErrorInvalidValue;
    switch (LA * 10 + LB) {
    case 12: return f(QMemberForm<1, 2, 64>{});
    case 21: return f(QMemberForm<2, 1, 64>{});
    case 22: return f(QMemberForm<2, 2, 64>{});
    case 13: return f(QMemberForm<1, 3, 64>{});
    case 31: return f(QMemberForm<3, 1, 64>{});
    case 23: return f(QMemberForm<2, 3, 64>{});
    case 32: return f(QMemberForm<3, 2, 64>{});
    case 33: return f(QMemberForm<3, 3, 64>{});
    default: return hipErrorInvalidValue;
    }
}

// one(form) launches a kernel of that form.  A 3 x 3 launch is the pair <3,3> + <2,2 on 3-plane storage> when a plane mask is present
// (k_mfma: each kernel of the pair reads the masks — the stack's or the launch's, the OR over every member — and returns at once
// unless it is the one that fits); with a chain both partners carry it, and the one the masks select stores D
template <class Form, class One>
hipError_t qg_member_launch(Form form, const QMfmaArgs& a, One&& one)
{
    const hipError_t e = one(form);
    if constexpr (Form::LA == 3 && Form::LB == 3) {
        if (e == hipSuccess && (a.maskA || a.maskB)) return one(QMemberForm<2, 2, Form::BK, 3, 3>{});
    }
    return e;
}

// the kernel K of a form: K<QG_MEMBER_FORM_ARGS(F)>
#define QG_MEMBER_FORM_ARGS(F) F::LA, F::LB, F::BK, F::WGM, F::WGN, F::TI, F::TJ, F::NSTAGE, F::SA, F::SB
