// clm_lab.h -- switches of lab builds (tools/build_variant.sh NAME -DCLM_LAB -DCLM_EXP_*): candidates measured against the product
// library with tools/abn.sh before anything is adopted.  The product build defines none of them and sees compile-time `false`s.
#pragma once

namespace clm {
namespace lab {

// CLM_EXP_NT=mask: which once-touched streams of the register-order fp16c tail kernel are non-temporal accesses (gemm16.hip NT_*:
// 1 h loads, 2 h stores, 4 y loads, 8 y-lo loads, 16 z stores, 32 z-lo stores; weight and bias loads never).  The product's mask is
// what same-box alternation kept (profiles/r06_h_order.txt): h loads AND stores together are the gain (tail kernel -2 %, 1.0 GB less
// fetch per launch; either alone, or the other four without them: nothing), the other four on top of them -0.8 % more.  In row
// order, where four instructions share every line of h, the same marks gained nothing -- the mask applies to the register-order
// instantiations only.
constexpr int NT_PRODUCT = 63;
#if defined(CLM_LAB) && defined(CLM_EXP_NT)
constexpr int NT_MASK = CLM_EXP_NT;
#else
constexpr int NT_MASK = NT_PRODUCT;
#endif

// CLM_EXP_HREG_BARRIER: the register-order form of the tail kernel keeps the barrier in front of its store of h (which it does not
// need): does the barrier's skew matter?
#if defined(CLM_LAB) && defined(CLM_EXP_HREG_BARRIER)
constexpr bool HREG_BARRIER = true;
#else
constexpr bool HREG_BARRIER = false;
#endif

}  // namespace lab
}  // namespace clm
