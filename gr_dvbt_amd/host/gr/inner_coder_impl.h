/* inner_coder_impl.h -- HIP-backed body of gr::dvbt::inner_coder (replaces lib/inner_coder_impl.h of gr-dvbt; see hip_shell.h) */
#ifndef INCLUDED_DVBT_INNER_CODER_IMPL_HIP_H
#define INCLUDED_DVBT_INNER_CODER_IMPL_HIP_H

#include <dvbt/inner_coder.h>
#include "hip_shell.h"

namespace gr {
  namespace dvbt {

    class inner_coder_impl : public inner_coder
    {
      DVBT_HIP_SHELL_MEMBERS(inner_coder)
    public:
      inner_coder_impl(int ninput, int noutput, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_code_rate_t coderate);
      ~inner_coder_impl() {}
    };

  } // namespace dvbt
} // namespace gr

#endif
