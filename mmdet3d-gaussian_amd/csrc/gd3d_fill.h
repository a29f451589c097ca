// gd3d_fill.h — the library's one buffer fill: fill_words_kernel and its launcher are defined in gd3d_loss.hip (a __global__
// kernel lives in exactly one translation unit); every other unit reaches it through this plain function.  Not exported (gd3d.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gd3d {

// Clears (or fills) small or large device buffers from a KERNEL, never with a memset node (see gd3d_loss.hip).
int fill_words(void* p, size_t bytes, unsigned value, hipStream_t s);   // bytes: a multiple of 4

}  // namespace gd3d
