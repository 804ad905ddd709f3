// kernels_edge.hip -- the two local halo families that only STORE ghost cells, and the one family that only LOADS, compiled as ONE
// translation unit and hence one code object of the library: kernels_fill.hip (halo fill: the ghost cells an update would write
// receive one value), kernels_reflect.hip (halo reflection: the ghost cells at a non-periodic edge receive the mirror image of the
// interior) and kernels_reduce.hip (interior reductions: sum, dot product and largest magnitude of a box of cells).  Fill and
// reflection are 138 KB of device code together, well below the size that matters (kernels_batch.h says why the kernels live in
// several code objects); the wall values, which came with this unit, have a code object of their own (kernels_wall.hip, 317 KB), and
// the library keeps the number of code objects it had.  The sources stay files of their own.
#include "kernels_fill.hip"
#include "kernels_reflect.hip"
#include "kernels_reduce.hip"
