// msn_poly.hpp -- the six coefficients of rf_mds' weight (include/rfops.h, "minimum density sampling"): a degree-5 polynomial
// for 2^-f on [0, 1), p(f) = c0 + f (c1 + f (c2 + f (c3 + f (c4 + f c5)))), evaluated in Horner form with a separate fp32
// multiply and add at every step.  Fitted once in float64 by interpolation at the six Chebyshev nodes of [0, 1]
// (0.5 + 0.5 cos((2 k + 1) pi / 12)) and rounded to fp32; tests/test_msn_ops_host.py mirrors this table (and reads this file
// to prove it) and holds the fp32 evaluation to 4 x (fit error) + 10 x 2^-24.
//
// Maximum relative error against exp2(-f) in float64 over the grid f = i / 2^20, i = 0 .. 2^20 - 1:
//   the fit before rounding, evaluated in float64               1.016e-7
//   these fp32 coefficients, evaluated in float64               1.024e-7
//   these fp32 coefficients, fp32 Horner (what the kernel runs) 2.61e-7
#pragma once

#define RF_MDS_POLY_C0 0x1.fffffep-1f
#define RF_MDS_POLY_C1 -0x1.62e3a8p-1f
#define RF_MDS_POLY_C2 0x1.ebe2f2p-3f
#define RF_MDS_POLY_C3 -0x1.c5009p-5f
#define RF_MDS_POLY_C4 0x1.2dc434p-7f
#define RF_MDS_POLY_C5 -0x1.f06faep-11f
