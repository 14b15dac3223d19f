// Stand-in for the header of that name that torch no longer ships: the atomics moved to ATen.
#include <ATen/cuda/Atomic.cuh>
