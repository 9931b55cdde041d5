/*
 * sde_geom.h -- C ABI of the geometry stage around the matching path (exported by the same libsde.so).
 *
 * The two ends of the pipeline that sde.h's matching path assumes done elsewhere:
 *   rectification of a raw camera pair from a calibration (Calibration/mycalibration.cpp:826-839:
 *   stereoRectify, initUndistortRectifyMap(..., CV_16SC2, ...), remap(..., INTER_LINEAR)), and
 *   reprojection of the disparity map to metric depth or an XYZ cloud (the GUI's `calculate`).
 * Chessboard detection and the estimation of a calibration are not here: a calibration is an input.
 *
 * Conventions are sde.h's: device pointers owned by the caller unless marked HOST, nothing allocates, frees or
 * synchronises, every call is stream-ordered and capturable into a hipGraph (HOST arrays are copied into the
 * kernel arguments by value and may be freed on return), `stream` is a hipStream_t passed as void*, the return
 * value is SDE_OK or a negative sde_status, and errors are detected before any launch (argument checks) or right
 * after it.  Every constant here is an integer literal.  The functions are additive: SDE_ABI_VERSION
 * stays 4.
 *
 * BUILD-DEFINED: the definitions below are stated in full and restated in NumPy under tests/ (bit-exact against
 * that restatement).  They follow OpenCV's pinhole + rational distortion model and its 5-bit INTER_LINEAR scheme
 * with a constant-0 border, restated in exact integers, but parity with OpenCV itself is unpinned (no OpenCV was
 * available to compare against), as for the cross-based aggregation of sde.h.
 */
#ifndef SDE_GEOM_H
#define SDE_GEOM_H

#include "sde.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A map entry whose source coordinate is not finite or not below 2^30 in magnitude (both words hold it). */
#define SDG_NO_SAMPLE -2147483648

/*
 * The fixed-point sampling map of one camera, built once per calibration.
 * cal (HOST, 26 doubles): K (9, row-major; K00 K01 K02 K11 K12 are used), dist (8: k1 k2 p1 p2 k3 k4 k5 k6,
 * OpenCV's order, zeros for absent terms), Minv (9, row-major) = inverse of P[:, :3] @ R of that camera's
 * rectification.  Thin-prism and tilt terms are not modelled.
 * For output pixel (u, v), in float64, every operation rounded on its own and evaluated as parenthesised:
 *   X = (Minv00*u + Minv01*v) + Minv02     (Y, Wd likewise from rows 1, 2)
 *   x = X/Wd; y = Y/Wd; xx = x*x; yy = y*y; xy = x*y; r2 = xx + yy
 *   kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
 *   xd = (x*kr + (2*p1)*xy) + p2*(r2 + 2*xx)
 *   yd = (y*kr + p1*(r2 + 2*yy)) + (2*p2)*xy
 *   us = (K00*xd + K01*yd) + K02;  vs = K11*yd + K12
 *   a = rint(us*32), b = rint(vs*32)        (round half to even)
 * map int32 [H][W][2]: map[v][u] = (a, b) if both are finite and below 2^30 in magnitude, else
 * (SDG_NO_SAMPLE, SDG_NO_SAMPLE).
 * SDE_ERR_ARG: a null cal or map, H or W < 1, H*W >= 2^30.
 */
int sdg_rectify_map(const double *cal, int H, int W, int32_t *map, void *stream);

/*
 * Bilinear resampling of nimg u8 images through their maps, in integers; image i reads src + i*Hs*Ws through
 * map + i*H*W*2 and writes dst + i*H*W (a stereo pair is one launch with nimg = 2, and dst can be the resident
 * [2][H][W] pair that sde_preprocess_u8_batch reads).  For a map entry (a, b):
 *   x0 = a >> 5 (arithmetic shift), fx = a & 31; y0, fy likewise from b;
 *   weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx*fy on taps (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1);
 *   a tap with zero weight is not read; a read tap outside the source contributes 0;
 *   dst = (sum w*p + 512) >> 10          (the weights sum to 1024: at most 255)
 *   valid = 1 iff every read tap is inside the source, else 0.
 * The first tap's weight is never zero, and an entry holding SDG_NO_SAMPLE in either word has that tap outside
 * any source: it gives dst = 0, valid = 0 by the same arithmetic, as does any int32 pair (no coordinate forms
 * an address before it has passed the inside test).  Every byte of dst is written, and every byte of valid
 * (optional, NULL to skip; u8 [nimg][H][W]) when given.  dst must not alias src.
 * SDE_ERR_ARG: a null src, map or dst, nimg or any size < 1, Hs*Ws or H*W >= 2^30, nimg > 65535.
 */
int sdg_remap_u8(const uint8_t *src, int nimg, int Hs, int Ws, const int32_t *map, int H, int W, uint8_t *dst,
                 uint8_t *valid, void *stream);

/*
 * Disparity -> depth and / or XYZ through the 4x4 reprojection matrix Q (HOST, 16 doubles, row-major).
 * disp float32 [H][W]; pixel (y, x) with d = disp[y][x] is valid iff d is finite and d > min_disp (float32
 * comparison; with min_disp >= 0 this excludes the -1 that means "no winner"; sub-pixel values are used as they
 * are).  For a valid pixel, in float64 with every operation rounded on its own,
 *   v_r = ((Q[r][0]*x + Q[r][1]*y) + Q[r][2]*d) + Q[r][3]          r = 0..3
 *   xyz[y][x] = float32(v0/v3), float32(v1/v3), float32(v2/v3);   depth[y][x] = float32(v2/v3)
 * as the arithmetic gives them (a zero v3 gives infinities or NaN).  An invalid pixel gets 0.0f in every output.
 * depth float32 [H][W] and xyz float32 [H][W][3] are each optional (NULL to skip), not both.
 * SDE_ERR_ARG: a null disp or Q, both outputs null, H or W < 1, H*W >= 2^30.
 */
int sdg_reproject(const float *disp, int H, int W, const double *Q, float min_disp, float *depth, float *xyz,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDE_GEOM_H */
