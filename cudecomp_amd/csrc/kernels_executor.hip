// kernels_executor.hip -- the two small kernel files the executors launch themselves, compiled as ONE translation unit and hence
// one code object of the library: kernels_rotate.hip (the in-place rotation, transpose.cc) and sync.hip (the signal / wait kernels
// of the one-sided exchanges).  Together they are 38 KB of device code, an order of magnitude below the size that matters
// (kernels_batch.h says why the kernels live in several code objects), and neither is on the path of a data-movement launch of the
// classifier.  Their sources are unchanged and stay files of their own.
#include "kernels_rotate.hip"
#include "sync.hip"
