/* dvbt_map_impl.cc -- gr::dvbt::dvbt_map on libdvbt_hip (replaces lib/dvbt_map_impl.cc).  Points: make_constellation_points scaled by gain * norm, hierarchical alpha included. */
#include "dvbt_map_impl.h"

namespace gr {
  namespace dvbt {

    dvbt_map::sptr
    dvbt_map::make(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission, float gain)
    { return gnuradio::get_initial_sptr(new dvbt_map_impl(nsize, constellation, hierarchy, transmission, gain)); }

    static dvbt_map_params map_params(int nsize, int constellation, int hierarchy, int transmission, float gain)
    { dvbt_map_params q = { nsize, constellation, hierarchy, transmission, gain }; return q; }

    /* io signatures and scheduler hints: lib/dvbt_map_impl.cc:44-47 */
    dvbt_map_impl::dvbt_map_impl(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission, float gain)
      : block("dvbt_map", io_signature::make(1, 1, sizeof(unsigned char) * nsize), io_signature::make(1, 1, sizeof(gr_complex) * nsize)),
        DVBT_HIP_CORE_INIT(map, map_params(nsize, constellation, hierarchy, transmission, gain))
    {
    }

  } /* namespace dvbt */
} /* namespace gr */
