// qgemul_reference_binding.hpp — the stub a QuBLAS maintainer would add to the reference header's
// "BLAS" section (after Reducer/Qreduce, /root/reference/include/QuBLAS.h:4899-5018) to get the README's
//     Qgemul<QgemulAddArgs<list>, QgemulMulArgs<type1>, QgemulTransposedA<true>>(m3, m1, m1);
// (readme.md:84-87) running on an MI355X through libqugemm.so.
//
// It must be included AFTER the reference's own QuBLAS.h: it contains no arithmetic and no tag
// machinery of its own — every result format is obtained from the reference's types by
// decltype on the reference's own Qmul / Qadd / Qsub front-ends (QuBLAS.h:3980-3999) and on the
// member typedefs of its complex multipliers (:3429-3435, :3513-3520), so the lowering cannot
// drift from the header it extends.  What it adds: the three Qgemul tags, the compile-time
// walk over the tree levels (Reducer::ReducerTypeSelector semantics, :4906-4921, :4966), and one
// call of the C-ABI entry point with the tensors' contiguous storage (Qu_s<dim<…>,T>::data.data(),
// column-major, :2680-2713).
//
// The repository's standalone header include/QuBLAS_amd.h provides the same Qgemul on its own
// minimal tag API for users who do not have the reference header.
#pragma once
#include <array>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>

#include "qgemul.h"

inline namespace QuBLAS {

template <typename... Args> struct QgemulAddArgs {};
template <typename... Args> struct QgemulMulArgs {};
template <bool Value> struct QgemulTransposedA { static constexpr bool value = Value; };

namespace qgemul_detail {

template <class T> constexpr qfmt fmt_of()
{
    return qfmt{int16_t(T::intB), int16_t(T::fracB), uint8_t(T::isS), uint8_t(T::QuM), uint8_t(T::OfM), 0};
}
template <class T, bool = T::is_complex> struct parts { using re = T; using im = T; };
template <class T> struct parts<T, true> { using re = typename T::realType; using im = typename T::imagType; };

// ---- optional, order-free Qgemul tags (same convention as every other tag pack in the header)
template <class... Tags> struct pick_add { using type = TypeList<>; };
template <class... L, class... Rest> struct pick_add<QgemulAddArgs<L...>, Rest...> { using type = TypeList<L...>; };
template <class... L, class... Rest> struct pick_add<QgemulAddArgs<TypeList<L...>>, Rest...> { using type = TypeList<L...>; };
template <class T, class... Rest> struct pick_add<T, Rest...> : pick_add<Rest...> {};

template <class... Tags> struct pick_mul { using type = TypeList<>; };
template <class... L, class... Rest> struct pick_mul<QgemulMulArgs<L...>, Rest...> { using type = TypeList<L...>; };
template <class T, class... Rest> struct pick_mul<T, Rest...> : pick_mul<Rest...> {};

template <class... Tags> struct pick_ta { static constexpr bool value = false; };
template <bool V, class... Rest> struct pick_ta<QgemulTransposedA<V>, Rest...> { static constexpr bool value = V; };
template <class T, class... Rest> struct pick_ta<T, Rest...> : pick_ta<Rest...> {};

template <class List> struct mul_with;
template <class... Tags> struct mul_with<TypeList<Tags...>> {
    template <class X, class Y> static auto go(const X& x, const Y& y) { return Qmul<Tags...>(x, y); }
};

// ---- product sub-operation formats
template <class EA, class EB, class MulList> struct slots;
template <class EA, class EB, class... Tags>
    requires(!EA::is_complex && !EB::is_complex)
struct slots<EA, EB, TypeList<Tags...>> {
    using prod_t = decltype(Qmul<Tags...>(std::declval<EA>(), std::declval<EB>()));
    static constexpr int cmul = QG_CMUL_NONE;
    static void fill(qgemul_desc& d) { d.mul[QG_MUL_REAL] = fmt_of<prod_t>(); }
};
// ONE real and ONE complex operand: the header's own part-wise Qmul(real, complex) / Qmul(complex, real) (QuBLAS.h:3604-3644)
// names the two product formats (realT / imagT tags, or two bare Qu types)
template <class EA, class EB, class... Tags>
    requires(EA::is_complex != EB::is_complex)
struct slots<EA, EB, TypeList<Tags...>> {
    using prod_t = decltype(Qmul<Tags...>(std::declval<EA>(), std::declval<EB>()));
    static constexpr int cmul = EA::is_complex ? QG_CMUL_REAL_B : QG_CMUL_REAL_A;
    static void fill(qgemul_desc& d) { d.mul[QG_M_RE] = fmt_of<typename prod_t::realType>(); d.mul[QG_M_IM] = fmt_of<typename prod_t::imagType>(); }
};
template <class EA, class EB, class... Args>
    requires(EA::is_complex && EB::is_complex)
struct slots<EA, EB, TypeList<BasicComplexMul<Args...>>> {
    using S = Qmul_s<EA, EB, BasicComplexMul<Args...>>;
    using a_t = typename EA::realType; using b_t = typename EA::imagType;
    using c_t = typename EB::realType; using d_t = typename EB::imagType;
    using ac_t = decltype(Qmul<typename S::mulACType>(std::declval<a_t>(), std::declval<c_t>()));
    using bd_t = decltype(Qmul<typename S::mulBDType>(std::declval<b_t>(), std::declval<d_t>()));
    using ad_t = decltype(Qmul<typename S::mulADType>(std::declval<a_t>(), std::declval<d_t>()));
    using bc_t = decltype(Qmul<typename S::mulBCType>(std::declval<b_t>(), std::declval<c_t>()));
    using re_t = decltype(Qsub<typename S::subACBDType>(std::declval<ac_t>(), std::declval<bd_t>()));
    using im_t = decltype(Qadd<typename S::addADBCType>(std::declval<ad_t>(), std::declval<bc_t>()));
    using prod_t = Qcomplex<re_t, im_t>;
    static constexpr int cmul = QG_CMUL_BASIC;
    static void fill(qfmt (&m)[8])
    {
        m[QG_B_AC] = fmt_of<ac_t>(); m[QG_B_BD] = fmt_of<bd_t>(); m[QG_B_AD] = fmt_of<ad_t>();
        m[QG_B_BC] = fmt_of<bc_t>(); m[QG_B_RE] = fmt_of<re_t>(); m[QG_B_IM] = fmt_of<im_t>();
    }
    static void fill(qgemul_desc& d) { fill(d.mul); }
};
template <class EA, class EB>
    requires(EA::is_complex && EB::is_complex)
struct slots<EA, EB, TypeList<>> : slots<EA, EB, TypeList<BasicComplexMul<>>> {}; // QuBLAS.h:3422-3424
template <class EA, class EB, class... Args>
    requires(EA::is_complex && EB::is_complex)
struct slots<EA, EB, TypeList<TFComplexMul<Args...>>> {
    using S = Qmul_s<EA, EB, TFComplexMul<Args...>>;
    using a_t = typename EA::realType; using b_t = typename EA::imagType;
    using c_t = typename EB::realType; using d_t = typename EB::imagType;
    using ab_t = decltype(Qadd<typename S::addabType>(std::declval<a_t>(), std::declval<b_t>()));
    using cd_t = decltype(Qadd<typename S::addcdType>(std::declval<c_t>(), std::declval<d_t>()));
    using ba_t = decltype(Qsub<typename S::subbaType>(std::declval<b_t>(), std::declval<a_t>()));
    using A_t = decltype(Qmul<typename S::mulabcType>(std::declval<ab_t>(), std::declval<c_t>()));
    using B_t = decltype(Qmul<typename S::mulbadType>(std::declval<cd_t>(), std::declval<b_t>()));
    using C_t = decltype(Qmul<typename S::mulcdbType>(std::declval<ba_t>(), std::declval<d_t>()));
    using re_t = decltype(Qsub<typename S::subABType>(std::declval<A_t>(), std::declval<B_t>()));
    using im_t = decltype(Qsub<typename S::subBCType>(std::declval<B_t>(), std::declval<C_t>()));
    using prod_t = Qcomplex<re_t, im_t>;
    static constexpr int cmul = QG_CMUL_TF;
    static void fill(qfmt (&m)[8])
    {
        m[QG_T_AB] = fmt_of<ab_t>(); m[QG_T_CD] = fmt_of<cd_t>(); m[QG_T_BA] = fmt_of<ba_t>();
        m[QG_T_A] = fmt_of<A_t>(); m[QG_T_B] = fmt_of<B_t>(); m[QG_T_C] = fmt_of<C_t>();
        m[QG_T_RE] = fmt_of<re_t>(); m[QG_T_IM] = fmt_of<im_t>();
    }
    static void fill(qgemul_desc& d) { fill(d.mul); }
};

// ---- tree levels: type of level l as Reducer selects it, formats of the add and of the buffer.
// The walk stops early once the buffer type repeats (all further levels are identical), so the
// template depth is bounded by the length of the level list, not by log2 K.
template <size_t L, class Prev, class List> struct level_sel;
template <size_t L, class Prev> struct level_sel<L, Prev, TypeList<>> { using tag = std::nullptr_t; using buf = Prev; };
template <size_t L, class Prev, class... Ls> struct level_sel<L, Prev, TypeList<Ls...>> {
    using tag = TypeAt<(L >= sizeof...(Ls) ? sizeof...(Ls) - 1 : L), TypeList<Ls...>>;
    using buf = tag;
};
template <size_t L, class Prev, class List>
void fill_levels(qgemul_desc& d)
{
    using sel = level_sel<L, Prev, List>;
    using add_t = decltype(Qadd<typename sel::tag>(std::declval<Prev>(), std::declval<Prev>()));
    using buf_t = typename sel::buf;
    constexpr size_t n_list = List::size;
    constexpr bool steady = std::is_same_v<buf_t, Prev> && (L + 1 >= n_list);
    const uint32_t last = steady ? d.n_levels : L + 1;
    for (uint32_t l = L; l < last && l < d.n_levels; ++l) {
        d.level_add[0][l] = fmt_of<typename parts<add_t>::re>();
        d.level_add[1][l] = fmt_of<typename parts<add_t>::im>();
        d.level[0][l] = fmt_of<typename parts<buf_t>::re>();
        d.level[1][l] = fmt_of<typename parts<buf_t>::im>();
    }
    if constexpr (!steady && L + 1 < QG_MAX_LEVELS) {
        if (L + 1 < d.n_levels) fill_levels<L + 1, buf_t, List>(d);
    }
}

} // namespace qgemul_detail

// lower a Qgemul call on reference tensor types to the C-ABI descriptor (no device access)
template <typename... Tags, size_t CM, size_t CN, size_t AR, size_t AC, size_t BK, size_t BN, class EC, class EA, class EB>
qgemul_desc Qgemul_lower_types(std::type_identity<Qu_s<dim<CM, CN>, EC>>, std::type_identity<Qu_s<dim<AR, AC>, EA>>,
                               std::type_identity<Qu_s<dim<BK, BN>, EB>>)
{
    using namespace qgemul_detail;
    constexpr bool ta = pick_ta<Tags...>::value;
    constexpr size_t M = ta ? AC : AR, K = ta ? AR : AC;
    static_assert(M == CM && BN == CN && BK == K, "Qgemul: C is MxN, A is MxK (KxM when transposed), B is KxN");
    // real x real -> real; complex x complex, real x complex and complex x real -> complex (the mixed forms: QG_CMUL_REAL_A / _B of qgemul.h)
    static_assert(EC::is_complex == (EA::is_complex || EB::is_complex), "Qgemul: C is complex exactly when an operand is");
    using mul_list = typename pick_mul<Tags...>::type;
    using add_list = typename pick_add<Tags...>::type;
    using S = slots<EA, EB, mul_list>;
    qgemul_desc d{};
    d.abi = QGEMUL_ABI_VERSION;
    d.transA = ta;
    d.is_complex = EC::is_complex;
    d.cmul = uint8_t(S::cmul);
    d.M = int64_t(M); d.N = int64_t(CN); d.K = int64_t(K);
    d.a[0] = fmt_of<typename parts<EA>::re>(); d.a[1] = fmt_of<typename parts<EA>::im>();
    d.b[0] = fmt_of<typename parts<EB>::re>(); d.b[1] = fmt_of<typename parts<EB>::im>();
    d.c[0] = fmt_of<typename parts<EC>::re>(); d.c[1] = fmt_of<typename parts<EC>::im>();
    if constexpr (EC::is_complex && !EA::is_complex) d.a[1] = qfmt{};   // a mixed descriptor's real operand: its format in [0], [1] all zero
    if constexpr (EC::is_complex && !EB::is_complex) d.b[1] = qfmt{};
    S::fill(d);
    for (size_t k = K; k > 1; k = (k + 1) / 2) ++d.n_levels;
    if (d.n_levels) fill_levels<0, typename S::prod_t, add_list>(d);
    return d;
}

template <typename... Tags, class TC, class TA, class TB>
qgemul_desc Qgemul_lower(const TC&, const TA&, const TB&)
{
    return Qgemul_lower_types<Tags...>(std::type_identity<TC>{}, std::type_identity<TA>{}, std::type_identity<TB>{});
}

// Options of the one-shot calls below, per translation unit (QG_OPT_* of qgemul.h).  Several GPUs in one process:
//     QgemulRunFlags() |= QG_OPT_ALL_DEVICES;     // every Qgemul<...>(C, A, B) is row-sharded over all visible gfx950 devices
// QgemulRelease() frees what the library caches for the calling thread (context, plan, device buffers); the library also does
// it when the thread exits.
inline uint32_t& QgemulRunFlags()
{
    static uint32_t flags = 0;
    return flags;
}
inline void QgemulRelease() { qgemul_run_release(); }
// Descriptor flags OR-ed into every lowered Qgemul of this translation unit.  QgemulDescFlags() |= QG_DESC_REFERENCE_ARTEFACTS asks
// for the reference's own result where that is an implementation artefact the engine otherwise refuses (qgemul.h: C of an unsigned
// WRP::TCPL format with exactly 32 value bits comes out unwrapped).
inline uint8_t& QgemulDescFlags()
{
    static uint8_t flags = 0;
    return flags;
}

// the README entry point: C = A' * B with per-product and per-tree-node quantisation
template <typename... Tags, class TC, class TA, class TB>
void Qgemul(TC& C, const TA& A, const TB& B)
{
    qgemul_desc d = Qgemul_lower<Tags...>(C, A, B);
    d.flags |= QgemulDescFlags();
    qgemul_opts opts{};
    opts.device = -1;
    opts.flags = QgemulRunFlags();
    const int st = qgemul_run(&d, C.data.data(), A.data.data(), B.data.data(), &opts);
    if (st != QG_OK) throw std::runtime_error(std::string("Qgemul: ") + qgemul_strerror(st));
}

// ---- batched Qgemul: `Bt` independent GEMMs of one descriptor on 3-d tensors ----
//     Qu<dim<M, N, Bt>, EC> C;  Qu<dim<M, K, Bt>, EA> A;  Qu<dim<K, N, Bt>, EB> B;     (A: dim<K, M, Bt> under QgemulTransposedA<true>)
//     QgemulBatched<tags...>(C, A, B);      // member b:  Qgemul<tags...>(C[:, :, b], A[:, :, b], B[:, :, b])
// The column-major index makes the members contiguous at stride rows * cols.  Same tags and same lowering as Qgemul: the
// descriptor is the one Qgemul lowers for ONE member (qgemul_run_batched, qgemul.h); small linear-class members run as one launch.
template <typename... Tags, size_t CM, size_t CN, size_t CB, size_t AR, size_t AC, size_t AB, size_t BR, size_t BN, size_t BB, class EC, class EA, class EB>
qgemul_desc QgemulBatched_lower_types(std::type_identity<Qu_s<dim<CM, CN, CB>, EC>>, std::type_identity<Qu_s<dim<AR, AC, AB>, EA>>,
                                      std::type_identity<Qu_s<dim<BR, BN, BB>, EB>>, int64_t* batch, int64_t* strides)
{
    static_assert(CB == AB && CB == BB && CB >= 1, "QgemulBatched: C, A and B hold the same number of members (their last extent)");
    *batch = int64_t(CB);
    strides[0] = int64_t(CM * CN);
    strides[1] = int64_t(AR * AC);
    strides[2] = int64_t(BR * BN);
    return Qgemul_lower_types<Tags...>(std::type_identity<Qu_s<dim<CM, CN>, EC>>{}, std::type_identity<Qu_s<dim<AR, AC>, EA>>{},
                                       std::type_identity<Qu_s<dim<BR, BN>, EB>>{});
}
// the member descriptor, the member count and the strides of C, A, B in elements
template <typename... Tags, class TC, class TA, class TB>
qgemul_desc QgemulBatched_lower(const TC&, const TA&, const TB&, int64_t* batch, int64_t* strides)
{
    return QgemulBatched_lower_types<Tags...>(std::type_identity<TC>{}, std::type_identity<TA>{}, std::type_identity<TB>{}, batch, strides);
}
template <typename... Tags, class TC, class TA, class TB>
void QgemulBatched(TC& C, const TA& A, const TB& B)
{
    int64_t batch = 0, strides[3] = {0, 0, 0};
    qgemul_desc d = QgemulBatched_lower<Tags...>(C, A, B, &batch, strides);
    d.flags |= QgemulDescFlags();
    qgemul_opts opts{};
    opts.device = -1;
    opts.flags = QgemulRunFlags();
    const int st = qgemul_run_batched(&d, batch, C.data.data(), A.data.data(), B.data.data(), strides[0], strides[1], strides[2], &opts);
    if (st != QG_OK) throw std::runtime_error(std::string("QgemulBatched: ") + qgemul_strerror(st));
}

// ---- grouped Qgemul: GEMMs of DIFFERENT dim<> in one call ----
//     QgemulGrouped<tags...>(std::tie(C0, C1, ...), std::tie(A0, A1, ...), std::tie(B0, B1, ...));   // member g: Qgemul<tags...>(Cg, Ag, Bg)
// on 2-d tensors of any dim<> and one element type per operand.  Each triple is lowered by the Qgemul lowering (a shape mismatch
// inside a triple stays a compile-time error) and the call is qgemul_run_grouped (qgemul.h): the small linear-class members of one
// launch key run as ONE launch, every other member on its own plan.
namespace qgemul_detail {
template <typename... Tags>
struct GroupedLower {
    template <class TupC, class TupA, class TupB, size_t... I>
    static std::array<qgemul_desc, sizeof...(I)> lower(const TupC& C, const TupA& A, const TupB& B, std::index_sequence<I...>)
    {
        return {{Qgemul_lower<Tags...>(std::get<I>(C), std::get<I>(A), std::get<I>(B))...}};
    }
};
} // namespace qgemul_detail
// the members' descriptors, in order
template <typename... Tags, class... TC, class... TA, class... TB>
std::array<qgemul_desc, sizeof...(TC)> QgemulGrouped_lower(const std::tuple<TC&...>& C, const std::tuple<TA&...>& A, const std::tuple<TB&...>& B)
{
    static_assert(sizeof...(TC) >= 1 && sizeof...(TC) == sizeof...(TA) && sizeof...(TC) == sizeof...(TB), "QgemulGrouped: as many As and Bs as Cs, at least one");
    return qgemul_detail::GroupedLower<Tags...>::lower(C, A, B, std::index_sequence_for<TC...>{});
}
template <typename... Tags, class... TC, class... TA, class... TB>
void QgemulGrouped(const std::tuple<TC&...>& C, const std::tuple<TA&...>& A, const std::tuple<TB&...>& B)
{
    constexpr size_t G = sizeof...(TC);
    std::array<qgemul_desc, G> d = QgemulGrouped_lower<Tags...>(C, A, B);
    for (auto& m : d) m.flags |= QgemulDescFlags();
    const std::array<void*, G> pc = std::apply([](auto&... t) { return std::array<void*, G>{{(void*)t.data.data()...}}; }, C);
    const std::array<const void*, G> pa = std::apply([](auto&... t) { return std::array<const void*, G>{{(const void*)t.data.data()...}}; }, A);
    const std::array<const void*, G> pb = std::apply([](auto&... t) { return std::array<const void*, G>{{(const void*)t.data.data()...}}; }, B);
    qgemul_opts opts{};
    opts.device = -1;
    opts.flags = QgemulRunFlags();
    const int st = qgemul_run_grouped(d.data(), int64_t(G), pc.data(), pa.data(), pb.data(), nullptr, nullptr, nullptr, &opts);
    if (st != QG_OK) throw std::runtime_error(std::string("QgemulGrouped: ") + qgemul_strerror(st));
}

// ---- element-wise operators after the GEMM (the header's lazy tensor operators, QuBLAS.h:3780-3877, :4079-4100) ----
//     Qgemul<…>(C, A, B);   Qu<dim<M,N>, T1> t = Qmul<t1…>(C, s);   Qu<dim<M,N>, DT> D = Qadd<t2…>(t, Bias);
// as ONE call that never stores C or t:
//     Qgemul<…, QgemulResult<CT>>(D, A, B, ThenMul<T1, t1…>(s), ThenAdd<void, t2…>(Bias));
// Every operator's result type is decltype of the header's own scalar Qmul / Qadd / Qsub<tags…> on the running element
// type and the operand's element type, so the chain resolves exactly as the three statements above do.
// After a COMPLEX Qgemul the same spelling takes complex operands for ThenAdd / ThenSub / ThenRsub (realT<…> / imagT<…>
// tags, QuBLAS.h:3549-3589) and real operands for all four (:3604-3707); the chain is lowered to the two part-wise
// chains of qgemul_epilogue_cplx.  ThenMul<Into, BasicComplexMul<…> | TFComplexMul<…> | nothing>(E) with a complex tensor or
// scalar E is the header's complex x complex Qmul (QuBLAS.h:3421-3534): a QG_EW_CMUL stage whose sub-operation formats are
// resolved by decltype on the header's own Qmul / Qadd / Qsub, as the GEMM's multiplier slots are; a chain that holds one
// goes through qgemul_run_epcx.  Qmul<M>(E, x), the operand first, is ThenRmul.
template <class CT> struct QgemulResult {};

namespace qgemul_detail {
template <int OP, bool XFIRST, class Into, class Operand, typename... Tags>
struct EwStage {
    const Operand& e;
    static constexpr int op = OP;
    static constexpr bool x_first = XFIRST;
    static constexpr bool scalar = isScalar<Operand>;
    template <class O, bool = isScalar<O>> struct elem { using type = O; };
    template <class O> struct elem<O, false> { using type = typename O::elem_t; };
    using e_t = typename elem<Operand>::type;
    template <class X> static auto apply(const X& x, const e_t& y)
    {
        if constexpr (OP == QG_EW_MUL) { if constexpr (XFIRST) return Qmul<Tags...>(x, y); else return Qmul<Tags...>(y, x); }
        else if constexpr (OP == QG_EW_ADD) { if constexpr (XFIRST) return Qadd<Tags...>(x, y); else return Qadd<Tags...>(y, x); }
        else { if constexpr (XFIRST) return Qsub<Tags...>(x, y); else return Qsub<Tags...>(y, x); }
    }
    template <class X> using r_t = decltype(apply(std::declval<X>(), std::declval<e_t>()));
    template <class X> using next_t = std::conditional_t<std::is_void_v<Into>, r_t<X>, Into>;
    // complex x complex Qmul on the running element type X: the multiplier's sub-operation formats, first argument first
    template <class X> using cmul_slots = std::conditional_t<XFIRST, slots<X, e_t, TypeList<Tags...>>, slots<e_t, X, TypeList<Tags...>>>;
};
template <class... Tags> struct pick_result { using type = void; };
template <class CT, class... Rest> struct pick_result<QgemulResult<CT>, Rest...> { using type = CT; };
template <class T, class... Rest> struct pick_result<T, Rest...> : pick_result<Rest...> {};

// ThenApprox<Into, ANUS::Segment<…>…>(): the header's own Segment types (QuBLAS.h:4853-4863) lowered to a qgemul_approx.  The raw value
// of a coefficient is what the header holds for it (c.data.data) — never a double.
template <class S> struct seg_lower;
template <double BP, auto... as>
struct seg_lower<ANUS::Segment<BP, as...>> {
    static_assert(sizeof...(as) >= 1 && sizeof...(as) <= QG_MAX_COEF, "1 .. QG_MAX_COEF coefficients");
    static qgemul_approx_seg lower()
    {
        qgemul_approx_seg g{};
        g.breakpoint = BP;
        g.n_coef = sizeof...(as);
        uint32_t i = 0;
        ((g.f[i] = fmt_of<std::remove_cvref_t<decltype(as)>>(), g.a[i] = int64_t(as.data.data), ++i), ...);
        return g;
    }
};
template <class Into, class... Segs>
struct ApproxStage {
    static_assert(sizeof...(Segs) >= 1 && sizeof...(Segs) <= QG_MAX_SEG, "1 .. QG_MAX_SEG segments");
    static constexpr bool approx = true;
    static constexpr bool scalar = true;
    static constexpr int op = QG_EW_APPROX;
    template <class X> using r_t = decltype(ANUS::Qapprox<Segs...>(std::declval<X>()));   // decltype(x)
    template <class X> using next_t = std::conditional_t<std::is_void_v<Into>, r_t<X>, Into>;
    static const qgemul_approx* table()
    {
        static const qgemul_approx t = [] {
            qgemul_approx q{};
            q.n_seg = sizeof...(Segs);
            uint32_t g = 0;
            ((q.seg[g++] = seg_lower<Segs>::lower()), ...);
            return q;
        }();
        return &t;
    }
};
template <class S> constexpr bool is_approx = requires { requires S::approx; };

// complex chains: stage k of the chain of part P (0 = real parts, 1 = imaginary parts) — include/qgemul.h's table
template <class X, class S> constexpr bool is_cmul = requires { requires S::e_t::is_complex && S::op == QG_EW_MUL && X::is_complex; };
// the qgemul_cmul records of a chain, in stage order (on[k]: stage k is a complex x complex multiplication)
struct CmulRecords {
    qgemul_cmul rec[QG_MAX_EW];
    bool on[QG_MAX_EW];
    void pointers(const qgemul_cmul* (&p)[QG_MAX_EW]) const { for (int k = 0; k < QG_MAX_EW; ++k) p[k] = on[k] ? &rec[k] : nullptr; }
};
template <class X> void fill_chain_cplx(qgemul_epilogue_cplx&, uint32_t, CmulRecords*) {}
template <class X, class S0, class... Ss>
void fill_chain_cplx(qgemul_epilogue_cplx& ep, uint32_t k, CmulRecords* cx)
{
    static_assert(!is_approx<S0>, "Qapprox is defined on real values only (QuBLAS.h:4868)");
    using e_t = typename S0::e_t;
    using r_t = typename S0::template r_t<X>;
    using n_t = typename S0::template next_t<X>;
    static_assert(X::is_complex && r_t::is_complex && n_t::is_complex, "a complex chain runs on complex tensors");
    ep.e_complex[k] = e_t::is_complex;
    qgemul_ew_stage& re = ep.part[0].stage[k];
    qgemul_ew_stage& im = ep.part[1].stage[k];
    re.op = im.op = uint8_t(S0::op);
    if constexpr (is_cmul<X, S0>) {   // r_t is the header's own Qmul result: the RE / IM slots by construction
        using M = typename S0::template cmul_slots<X>;
        static_assert(std::is_same_v<typename M::prod_t, r_t>);
        re.op = im.op = uint8_t(QG_EW_CMUL);
        if (cx) {
            cx->rec[k].cmul = uint8_t(M::cmul);
            M::fill(cx->rec[k].mul);
            cx->on[k] = true;
        }
    }
    re.x_first = im.x_first = S0::x_first;
    re.e_scalar = im.e_scalar = S0::scalar;
    re.e = fmt_of<typename parts<e_t>::re>();
    im.e = fmt_of<typename parts<e_t>::im>();
    re.r = fmt_of<typename r_t::realType>();
    im.r = fmt_of<typename r_t::imagType>();
    re.t = fmt_of<typename n_t::realType>();
    im.t = fmt_of<typename n_t::imagType>();
    if constexpr (!e_t::is_complex && S0::op != QG_EW_MUL) {
        if constexpr (S0::op == QG_EW_ADD || S0::x_first) im.op = QG_EW_PASS;   // the imaginary part is carried over (QuBLAS.h:3654, :3670, :3701)
        im.e_scalar = 1;                                                        // real - complex: the zero of the operand's type (:3686)
    }
    fill_chain_cplx<n_t, Ss...>(ep, k + 1, cx);
}
template <class X> constexpr bool chain_has_cmul() { return false; }
template <class X, class S0, class... Ss> constexpr bool chain_has_cmul()
{
    if constexpr (is_approx<S0>) return false;
    else return is_cmul<X, S0> || chain_has_cmul<typename S0::template next_t<X>, Ss...>();
}

template <class X> void fill_chain(qgemul_epilogue&, uint32_t) {}
template <class X, class S0, class... Ss>
void fill_chain(qgemul_epilogue& ep, uint32_t k)
{
    using r_t = typename S0::template r_t<X>;
    using n_t = typename S0::template next_t<X>;
    ep.stage[k].op = uint8_t(S0::op);
    if constexpr (!is_approx<S0>) {   // (an APPROX stage: e, e_scalar and x_first stay zero)
        ep.stage[k].x_first = S0::x_first;
        ep.stage[k].e_scalar = S0::scalar;
        ep.stage[k].e = fmt_of<typename S0::e_t>();
    }
    ep.stage[k].r = fmt_of<r_t>();
    ep.stage[k].t = fmt_of<n_t>();
    fill_chain<n_t, Ss...>(ep, k + 1);
}
} // namespace qgemul_detail

template <class Into = void, typename... Tags, class Operand> auto ThenMul(const Operand& e) { return qgemul_detail::EwStage<QG_EW_MUL, true, Into, Operand, Tags...>{e}; }
template <class Into = void, typename... Tags, class Operand> auto ThenAdd(const Operand& e) { return qgemul_detail::EwStage<QG_EW_ADD, true, Into, Operand, Tags...>{e}; }
template <class Into = void, typename... Tags, class Operand> auto ThenSub(const Operand& e) { return qgemul_detail::EwStage<QG_EW_SUB, true, Into, Operand, Tags...>{e}; }
template <class Into = void, typename... Tags, class Operand> auto ThenRsub(const Operand& e) { return qgemul_detail::EwStage<QG_EW_SUB, false, Into, Operand, Tags...>{e}; }
template <class Into = void, typename... Tags, class Operand> auto ThenRmul(const Operand& e) { return qgemul_detail::EwStage<QG_EW_MUL, false, Into, Operand, Tags...>{e}; }
template <class Into, class... Segments> auto ThenApprox() { return qgemul_detail::ApproxStage<Into, Segments...>{}; }
// the tables of a chain, in stage order: the stage's qgemul_approx, nullptr for a stage that is no ThenApprox
template <class... Stages>
std::array<const qgemul_approx*, QG_MAX_EW> Qgemul_lower_approx(const Stages&...)
{
    std::array<const qgemul_approx*, QG_MAX_EW> t{};
    uint32_t k = 0;
    ([&] { if constexpr (qgemul_detail::is_approx<Stages>) t[k] = Stages::table(); ++k; }(), ...);
    return t;
}

template <typename... Tags, class TD, class... Stages>
qgemul_epilogue_cplx Qgemul_lower_epilogue_cplx_x(qgemul_detail::CmulRecords* cx, std::type_identity<TD>, std::type_identity<Stages>...)
{
    using CT = typename qgemul_detail::pick_result<Tags...>::type;
    static_assert(!std::is_void_v<CT>, "Qgemul with element-wise operators needs QgemulResult<CT>: the element type of the Qgemul result");
    static_assert(sizeof...(Stages) <= QG_MAX_EW, "at most QG_MAX_EW element-wise operators");
    static_assert(CT::is_complex && TD::elem_t::is_complex, "a complex chain runs from a complex Qgemul result into a complex tensor");
    qgemul_epilogue_cplx ep{};
    ep.part[0].n_stages = ep.part[1].n_stages = sizeof...(Stages);
    if (cx) *cx = qgemul_detail::CmulRecords{};
    qgemul_detail::fill_chain_cplx<CT, Stages...>(ep, 0, cx);
    ep.part[0].d = qgemul_detail::fmt_of<typename TD::elem_t::realType>();
    ep.part[1].d = qgemul_detail::fmt_of<typename TD::elem_t::imagType>();
    return ep;
}

template <typename... Tags, class TD, class... Stages>
qgemul_epilogue Qgemul_lower_epilogue(const TD&, const Stages&...)
{
    using CT = typename qgemul_detail::pick_result<Tags...>::type;
    static_assert(!std::is_void_v<CT>, "Qgemul with element-wise operators needs QgemulResult<CT>: the element type of the Qgemul result");
    static_assert(sizeof...(Stages) <= QG_MAX_EW, "at most QG_MAX_EW element-wise operators");
    static_assert(!CT::is_complex && !TD::elem_t::is_complex, "a complex chain is lowered by Qgemul_lower_epilogue_cplx");
    qgemul_epilogue ep{};
    ep.n_stages = sizeof...(Stages);
    qgemul_detail::fill_chain<CT, Stages...>(ep, 0);
    ep.d = qgemul_detail::fmt_of<typename TD::elem_t>();
    return ep;
}

template <typename... Tags, class TD, class... Stages>
qgemul_epilogue_cplx Qgemul_lower_epilogue_cplx(const TD&, const Stages&...)
{
    return Qgemul_lower_epilogue_cplx_x<Tags...>(static_cast<qgemul_detail::CmulRecords*>(nullptr), std::type_identity<TD>{}, std::type_identity<Stages>{}...);
}
// the qgemul_cmul record of every complex x complex ThenMul / ThenRmul of the chain, for the _epcx entry points
template <typename... Tags, class TD, class... Stages>
qgemul_detail::CmulRecords Qgemul_lower_cmul(const TD&, const Stages&...)
{
    qgemul_detail::CmulRecords cx;
    Qgemul_lower_epilogue_cplx_x<Tags...>(&cx, std::type_identity<TD>{}, std::type_identity<Stages>{}...);
    return cx;
}

template <typename... Tags, class TD, class TA, class TB, class S0, class... Stages>
void Qgemul(TD& D, const TA& A, const TB& B, const S0& s0, const Stages&... st)
{
    using CT = typename qgemul_detail::pick_result<Tags...>::type;
    static_assert(!std::is_void_v<CT>, "Qgemul with element-wise operators needs QgemulResult<CT>");
    qgemul_desc d = Qgemul_lower_types<Tags...>(std::type_identity<Qu_s<typename TD::size, CT>>{}, std::type_identity<TA>{}, std::type_identity<TB>{});
    d.flags |= QgemulDescFlags();
    auto ptr = [](const auto& stage) -> const void* {
        // a scalar is one element as the tensors store them (ArbiInt<N>::data, QuBLAS.h:353; {real, imag} for a complex one, :2512-2513)
        if constexpr (qgemul_detail::is_approx<std::remove_cvref_t<decltype(stage)>>) return nullptr;   // reads no operand
        else if constexpr (std::remove_cvref_t<decltype(stage)>::scalar) return &stage.e;
        else return stage.e.data.data();
    };
    const void* E[QG_MAX_EW] = {ptr(s0), ptr(st)...};
    int rc;
    if constexpr (CT::is_complex) {
        qgemul_detail::CmulRecords cx;
        const qgemul_epilogue_cplx ep = Qgemul_lower_epilogue_cplx_x<Tags...>(&cx, std::type_identity<TD>{}, std::type_identity<S0>{}, std::type_identity<Stages>{}...);
        if constexpr (qgemul_detail::chain_has_cmul<CT, S0, Stages...>()) {
            const qgemul_cmul* pcx[QG_MAX_EW];
            cx.pointers(pcx);
            rc = qgemul_run_epcx(&d, &ep, pcx, D.data.data(), A.data.data(), B.data.data(), E, nullptr);
        } else
            rc = qgemul_run_epc(&d, &ep, D.data.data(), A.data.data(), B.data.data(), E, nullptr);
    } else {
        const qgemul_epilogue ep = Qgemul_lower_epilogue<Tags...>(D, s0, st...);
        if constexpr (qgemul_detail::is_approx<S0> || (qgemul_detail::is_approx<Stages> || ...)) {
            const auto ax = Qgemul_lower_approx(s0, st...);
            rc = qgemul_run_epx(&d, &ep, ax.data(), D.data.data(), A.data.data(), B.data.data(), E, nullptr);
        } else {
            rc = qgemul_run_ep(&d, &ep, D.data.data(), A.data.data(), B.data.data(), E, nullptr);
        }
    }
    if (rc != QG_OK) throw std::runtime_error(std::string("Qgemul: ") + qgemul_strerror(rc));
}

} // namespace QuBLAS
