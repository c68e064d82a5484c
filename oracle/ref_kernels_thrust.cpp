// oracle/ref_kernels_thrust.cpp — TEST INFRASTRUCTURE ONLY (golden generation), companion of ref_kernels_harness.cpp.
//
// rocThrust's <thrust/random.h> pulls in rocPRIM and the HIP runtime's headers and does not compile under plain g++, while
// the reference's kernel bodies do not compile under hipcc's host pass with the stand-ins ref_kernels_harness.cpp uses.  So
// the two live in two objects: this one, compiled with `hipcc -x hip --cuda-host-only -fPIE -c`, holds the genuine
// thrust::default_random_engine and thrust::uniform_real_distribution<float> behind three C functions; the harness forwards
// a minimal `namespace thrust` to them and the link is done with g++ (nothing of the HIP runtime is needed at link time:
// the engine and the distribution are header-only integer / float arithmetic).
//
// The engine lives in 16 bytes of caller storage (it is one 32-bit word today; the assert below guards the margin), so the
// harness's stand-in type stays trivially copyable, as `auto rng = makeSeededRandomEngine(...)` (pathtrace.cu:368) needs.
#include <thrust/random.h>

#include <new>
#include <type_traits>

static_assert(sizeof(thrust::default_random_engine) <= 16, "engine does not fit the caller's storage");
static_assert(std::is_trivially_copyable<thrust::default_random_engine>::value, "engine is copied as bytes");

extern "C" {

// thrust::default_random_engine(h), constructed from an int as pathtrace.cu:206 does
void ref_thrust_seed(void* storage16, int h) { new (storage16) thrust::default_random_engine(h); }

// one raw engine output
unsigned ref_thrust_next(void* storage16) { return (unsigned)(*static_cast<thrust::default_random_engine*>(storage16))(); }

// thrust::uniform_real_distribution<float> u01(0.0f, 1.0f) applied to the engine (pathtrace.cu:369; the distribution is stateless)
float ref_thrust_u01(void* storage16) {
  thrust::uniform_real_distribution<float> u01(0.0f, 1.0f);
  return u01(*static_cast<thrust::default_random_engine*>(storage16));
}

}  // extern "C"
