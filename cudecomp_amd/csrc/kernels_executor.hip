// kernels_executor.hip -- the small kernel files compiled as ONE translation unit and hence one code object of the library:
// kernels_rotate.hip (the in-place rotation, transpose.cc) and sync.hip (the signal / wait kernels of the one-sided exchanges),
// which the executors launch themselves -- together 38 KB of device code, an order of magnitude below the size that matters
// (kernels_batch.h says why the kernels live in several code objects) -- and kernels_field_wall.hip (the wall field-moves of the
// multi-field wall values), which found no room in kernels_wall.hip or kernels_field_mirror.hip and joins the smallest unit
// instead, the way kernels_edge.hip joins fill and reflect.  DESIGN.md has the resulting size.  The sources stay files of their own.
#include "kernels_rotate.hip"
#include "sync.hip"
#include "kernels_field_wall.hip"
