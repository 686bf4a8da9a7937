// Device-side helpers every kernel file used to carry a copy of: the vector types of MFMA operands and 8 / 16-byte memory
// accesses, the buffer resource of a tensor and the LDS barrier.  Device code only -- ellifit_core.h and jpeg_decode_core.h, which
// the tests also compile into host programs, must not pull this in.
#pragma once

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr;

// Byte offset of a lane that must read zeros / drop its store: beyond num_records of any resource make_rsrc builds, so the buffer
// unit's range check takes care of it (out-of-image pixels, padded channels) without a branch.
constexpr unsigned OOB = 0x80000000u;

// Raw buffer resource over `bytes` bytes at `base` (stride 0: the range check compares the byte offset with num_records).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// Workgroup barrier that waits for this wave's LDS traffic only: global loads in flight (vmcnt) stay in flight across it, which
// __syncthreads() would drain.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
