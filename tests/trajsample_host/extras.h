// What csrc/mlpg_trajsample.hip needs beyond tests/gmm_host/common.h (tests/test_trajsample_host_cpu.py): what csrc/assemble.h and
// csrc/device_prims.h need -- tests/gvmlpg_host/extras.h, which the test copies next to this file as gvmlpg_extras.h: the
// structures and checks of csrc/common.h that the entry points use, and stand-ins for the device-only builtins that
// device_prims.h names in functions the text never calls.  Included behind common.h and in front of the kernel text.
#pragma once
#include "gvmlpg_extras.h"
#include <atomic>
#include <cstdint>
