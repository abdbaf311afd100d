// The fp16 ring (fp16_ring.inc) fed from the split's planes, textually included into pairdist_tile_kernel and pairdist_rows_tile_kernel
// (pairdist.hip): both operands are row blocks of P, and K runs over the three products hi.hi, hi.lo, lo.hi.
// Expects in scope, besides what fp16_ring.inc expects: p (T = Dp / 64), the descriptors rs0 (zero extent), rsA, rsW of the tile's row and
//   column block, and voff[4][2], the stager's lane offsets per half-tile kind -- what the kernel's set_tile points at a tile.
// Defines: nT, ring_src, and what fp16_ring.inc defines.
const int nT = 3 * p.T;                                          // K tiles of the three products: hi.hi, hi.lo, lo.hi
// K tile t of half-tile kind `kind`: its K tile inside P's row (hi | lo); tiles past the end go through the zero-extent descriptor
auto ring_src = [&](int kind, int t, __amdgpu_buffer_rsrc_t& rs, unsigned (&vo)[2], unsigned& so) {
    const bool isA = kind == 0 || kind == 3, valid = t < nT;
    rs = valid ? (isA ? rsA : rsW) : rs0;
    const int kt = isA ? (t < p.T ? t : t - p.T) : (t < 2 * p.T ? t : t - 2 * p.T);
    vo[0] = voff[kind][0]; vo[1] = voff[kind][1];
    so = (unsigned)kt * 128u;
};
#include "fp16_ring.inc"
