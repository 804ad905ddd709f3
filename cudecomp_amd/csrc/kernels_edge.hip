// kernels_edge.hip -- the two local halo families that only STORE ghost cells, compiled as ONE translation unit and hence one
// code object of the library: kernels_fill.hip (halo fill: the ghost cells an update would write receive one value) and
// kernels_reflect.hip (halo reflection: the ghost cells at a non-periodic edge receive the mirror image of the interior).  Together
// they are 138 KB of device code, well below the size that matters (kernels_batch.h says why the kernels live in several code
// objects); the wall values, which came with this unit, have a code object of their own (kernels_wall.hip, 317 KB), and the library
// keeps the number of code objects it had.  Both sources are unchanged and stay files of their own.
#include "kernels_fill.hip"
#include "kernels_reflect.hip"
