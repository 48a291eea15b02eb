// kernels.hip.h -- gfx950 device kernels of the tomography hot path.
//
// Device layout ("slab-interleaved"): every field is stored with the slice index
// fastest,   volume  x[pixel = y*N + z][s]   and   sinogram  g[row = angle*N + ray][s],   row pitch sx floats
// (sx = Nslice rounded up to 64, padding slices are identically zero).  All slices share one system
// matrix, so a matrix entry (row, pixel, w) is wave-uniform scalar data and its use is one coalesced
// vector AXPY across slices: lanes index slices, the scalar unit walks the ray / voxel tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The kernels live in one header per family; the order matters (constants and helpers are shared downwards):
#include "kernels_common.hip.h"   // vector helpers, reductions, transposes, the register-block typedefs
#include "kernels_fp.hip.h"       // forward projectors (defines row_ror, the FT_ tile shape)
#include "kernels_bp.hip.h"       // back projectors (defines CellD; k_bp_tile reuses the FT_ tile shape)
#include "kernels_sart.hip.h"     // streamed SART / ART sweeps (use CellD, row_ror, FT_BATCH)
#include "kernels_misc.hip.h"     // element-wise passes, reductions, multimodal, CGLS scalars, WBP filter
#include "kernels_tv.hip.h"       // TV value / gradient / update
#include "kernels_fgp.hip.h"      // FGP-TV
#include "kernels_pdhg.hip.h"     // Chambolle-Pock: dual sinogram, fused dual / divergence / primal pass
#include "kernels_geom.hip.h"     // shared by the families below: axis split, bilinear / trilinear value, two-stage sums
#include "kernels_align.hip.h"    // tilt-series alignment: moments, windowed cross-correlation, resampling
#include "kernels_align_normal.hip.h" // per-projection similarity matching: gather, gradient and the 4 x 4 normal equations in one pass
#include "kernels_tilt.hip.h"     // tilt-angle refinement: the rotational derivative of a volume, the per-projection sums of the angle step
#include "kernels_condition.hip.h" // conditioning of a tilt series: window statistics, local median, gain and offset
#include "kernels_markers.hip.h"  // marker detection: template NCC of every projection, local maxima with their neighbours
#include "kernels_bin.hip.h"      // binning of sinograms and volumes by 2 or 4, trilinear prolongation
#include "kernels_dual.hip.h"     // dual-axis: the volume transposed between two engines with perpendicular tilt axes
#include "kernels_affine3d.hip.h" // a volume resampled by a 3-D affine map (trilinear, binary64 coordinates)
#include "kernels_register3d.hip.h" // rigid registration of two volumes: gather, gradient and the 6 x 6 normal equations in one pass
#include "kernels_dart.hip.h"    // DART: label / boundary / free-set stencil, masked restore and smoother, per-class sums
#include "kernels_components.hip.h" // connected components: union-find labelling, renumbering scan, integer measurements, removal
