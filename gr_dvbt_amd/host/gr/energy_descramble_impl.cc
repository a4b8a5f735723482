/* energy_descramble_impl.cc -- gr::dvbt::energy_descramble on libdvbt_hip (replaces lib/energy_descramble_impl.cc).
 * Items are ALWAYS 8 packets of 188 bytes, whatever make() is given: the reference's d_nblocks is a constant 8 (:40) and its constructor never reads the
 * argument (:78-87), and dvbt_energy_descramble_work counts in items of 1504 bytes.  An item size taken from the argument would let the library read 1504
 * bytes of every 188 * nblocks the scheduler handed over. */
#include "energy_descramble_impl.h"

namespace gr {
  namespace dvbt {

    energy_descramble::sptr
    energy_descramble::make(int nblocks)
    { return gnuradio::get_initial_sptr(new energy_descramble_impl(nblocks)); }

    static const int ED_NBLOCKS = 8;

    static dvbt_energy_descramble_params ed_params(int)
    { dvbt_energy_descramble_params p = { ED_NBLOCKS }; return p; }

    /* io signatures, rate and output multiple: lib/energy_descramble_impl.cc:79-87 (items of 8 packets of 188 bytes in, bytes out) */
    energy_descramble_impl::energy_descramble_impl(int nblocks)
      : block("energy_descramble", io_signature::make(1, 1, sizeof(unsigned char) * ED_NBLOCKS * 188), io_signature::make(1, 1, sizeof(unsigned char))),
        DVBT_HIP_CORE_INIT(energy_descramble, ed_params(nblocks))
    {
      set_relative_rate((double)(ED_NBLOCKS * 188));
      set_output_multiple(4 * ED_NBLOCKS * 188);
    }

  } /* namespace dvbt */
} /* namespace gr */
