/* Stand-in for gr_expj: cos and sin in float (third-party arithmetic, restated). */
#ifndef REF_STANDIN_GR_EXPJ_H
#define REF_STANDIN_GR_EXPJ_H
#include <gnuradio/types.h>

static inline gr_complex gr_expj(float phase) { return gr_complex(cosf(phase), sinf(phase)); }
#endif
