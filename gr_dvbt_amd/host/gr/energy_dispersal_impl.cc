/* energy_dispersal_impl.cc -- gr::dvbt::energy_dispersal on libdvbt_hip (replaces lib/energy_dispersal_impl.cc).  The SYNC search reads the window back to the host on every call (include/dvbt_hip.h T1). */
#include "energy_dispersal_impl.h"

namespace gr {
  namespace dvbt {

    energy_dispersal::sptr
    energy_dispersal::make(int nsize)
    { return gnuradio::get_initial_sptr(new energy_dispersal_impl(nsize)); }

    static dvbt_energy_dispersal_params energy_dispersal_params(int nsize)
    { dvbt_energy_dispersal_params q = { nsize }; return q; }

    /* io signatures and scheduler hints: lib/energy_dispersal_impl.cc:71-77 */
    energy_dispersal_impl::energy_dispersal_impl(int nsize)
      : block("energy_dispersal", io_signature::make(1, 1, sizeof(unsigned char)), io_signature::make(1, 1, sizeof(unsigned char) * nsize * 8 * 188)),
        DVBT_HIP_CORE_INIT(energy_dispersal, energy_dispersal_params(nsize))
    {
      set_relative_rate(1.0 / (double)(nsize * 8 * 188));
    }

  } /* namespace dvbt */
} /* namespace gr */
