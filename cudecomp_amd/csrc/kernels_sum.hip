// kernels_sum.hip -- the two families of the halo accumulation, compiled as ONE translation unit and hence one code object of the
// library: kernels_accumulate.hip (add-moves: dst += src) and kernels_take.hip (take-moves: the copy or the addition, then zero
// bytes into the source cells).  Together they are 340 KB of device code, below the size that matters (kernels_batch.h says why the
// kernels live in several code objects); the wall planes, which came with this unit, have a code object of their own
// (kernels_wall_plane.hip, 320 KB), and the library keeps the number of code objects it had.  Both sources are unchanged and stay
// files of their own.
#include "kernels_accumulate.hip"
#include "kernels_take.hip"
