// longread_plan.h -- what csrc/longread_plan.cpp (plain C++, no HIP) shares with csrc/longread.hip and with a stand-alone program.
#pragma once
#include <string>

#include "chimeralm_hip.h"

namespace clm {
namespace longread {

constexpr unsigned char PAD_ID = 4, SEP_ID = 1;   // the reference's tokenizer: [PAD] = 4, [SEP] = 1

// The text behind clm_longread_last_error(NULL): the last failed clm_longread_lengths / _plan / _create.
std::string& host_error();

}  // namespace longread
}  // namespace clm
