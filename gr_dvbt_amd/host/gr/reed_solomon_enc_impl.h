/* reed_solomon_enc_impl.h -- HIP-backed body of gr::dvbt::reed_solomon_enc (replaces lib/reed_solomon_enc_impl.h of gr-dvbt; see hip_shell.h) */
#ifndef INCLUDED_DVBT_REED_SOLOMON_ENC_IMPL_HIP_H
#define INCLUDED_DVBT_REED_SOLOMON_ENC_IMPL_HIP_H

#include <dvbt/reed_solomon_enc.h>
#include "hip_shell.h"

namespace gr {
  namespace dvbt {

    class reed_solomon_enc_impl : public reed_solomon_enc
    {
      DVBT_HIP_SHELL_MEMBERS(reed_solomon_enc)
    public:
      reed_solomon_enc_impl(int p, int m, int gfpoly, int n, int k, int t, int s, int blocks);
      ~reed_solomon_enc_impl() {}
    };

  } // namespace dvbt
} // namespace gr

#endif
