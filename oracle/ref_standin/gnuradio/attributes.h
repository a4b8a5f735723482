/* Stand-in for GNU Radio's attributes.h: symbol-visibility macros only.
 * Written from scratch for oracle/Makefile target `ref` (see ref_standin/README.md). */
#ifndef REF_STANDIN_GR_ATTRIBUTES_H
#define REF_STANDIN_GR_ATTRIBUTES_H
#define __GR_ATTR_EXPORT __attribute__((visibility("default")))
#define __GR_ATTR_IMPORT __attribute__((visibility("default")))
#define __GR_ATTR_ALIGNED(x) __attribute__((aligned(x)))
#endif
