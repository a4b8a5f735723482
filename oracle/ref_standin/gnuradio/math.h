/* Stand-in for GNU Radio's math.h: the blocks in scope include it and use only <cmath> from it. */
#ifndef REF_STANDIN_GR_MATH_H
#define REF_STANDIN_GR_MATH_H
#include <gnuradio/types.h>
#endif
