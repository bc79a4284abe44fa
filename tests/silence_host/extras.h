// What csrc/frame_keep.hip needs beyond tests/gmm_host/common.h (tests/test_silence_host_cpu.py): nothing but the shim's typed
// shuffles (the scan moves long long sums) -- its constants come from include/nnmnkwii_silence.h and include/nnmnkwii_frontend.h,
// which the test copies next to the text.  Included behind common.h and in front of the kernel text.
#pragma once
#include "common.h"
#include <cstdint>
