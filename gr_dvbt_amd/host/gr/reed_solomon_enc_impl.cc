/* reed_solomon_enc_impl.cc -- gr::dvbt::reed_solomon_enc on libdvbt_hip (replaces lib/reed_solomon_enc_impl.cc).  Only the DVB parameter set (2,8,0x11d,255,239,8,51) is accepted. */
#include "reed_solomon_enc_impl.h"

namespace gr {
  namespace dvbt {

    reed_solomon_enc::sptr
    reed_solomon_enc::make(int p, int m, int gfpoly, int n, int k, int t, int s, int blocks)
    { return gnuradio::get_initial_sptr(new reed_solomon_enc_impl(p, m, gfpoly, n, k, t, s, blocks)); }

    static dvbt_reed_solomon_enc_params reed_solomon_enc_params(int p, int m, int gfpoly, int n, int k, int t, int s, int blocks)
    { dvbt_reed_solomon_enc_params q = { p, m, gfpoly, n, k, t, s, blocks }; return q; }

    /* io signatures and scheduler hints: lib/reed_solomon_enc_impl.cc:43-47 */
    reed_solomon_enc_impl::reed_solomon_enc_impl(int p, int m, int gfpoly, int n, int k, int t, int s, int blocks)
      : block("reed_solomon", io_signature::make(1, 1, sizeof(unsigned char) * blocks * (k - s)), io_signature::make(1, 1, sizeof(unsigned char) * blocks * (n - s))),
        DVBT_HIP_CORE_INIT(reed_solomon_enc, reed_solomon_enc_params(p, m, gfpoly, n, k, t, s, blocks))
    {
    }

  } /* namespace dvbt */
} /* namespace gr */
