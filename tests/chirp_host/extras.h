// What csrc/modspec_chirp.hip needs beyond tests/gmm_host/common.h and what csrc/modspec_fft.h needs already
// (tests/msfilter_host/extras.h, which the test copies here as fft_extras.h): the out-of-memory code.  double2 and the stand-in
// for mlpg::scratch() are the shim's.  Included behind common.h and in front of the kernel text.
#pragma once
#include "fft_extras.h"
#define MLPG_HIP_ENOMEM (-3)
