/* bit_inner_interleaver_impl.cc -- gr::dvbt::bit_inner_interleaver on libdvbt_hip (replaces lib/bit_inner_interleaver_impl.cc).  Non-hierarchical only: one input (the reference's io_signature(1, 2)); hierarchy != NH is refused (include/dvbt_hip.h T5). */
#include "bit_inner_interleaver_impl.h"

namespace gr {
  namespace dvbt {

    bit_inner_interleaver::sptr
    bit_inner_interleaver::make(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission)
    { return gnuradio::get_initial_sptr(new bit_inner_interleaver_impl(nsize, constellation, hierarchy, transmission)); }

    static dvbt_bit_inner_interleaver_params bit_inner_interleaver_params(int nsize, int constellation, int hierarchy, int transmission)
    { dvbt_bit_inner_interleaver_params q = { nsize, constellation, hierarchy, transmission }; return q; }

    /* io signatures and scheduler hints: lib/bit_inner_interleaver_impl.cc:71-74 */
    bit_inner_interleaver_impl::bit_inner_interleaver_impl(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission)
      : block("bit_inner_interleaver", io_signature::make(1, 1, sizeof(unsigned char) * nsize), io_signature::make(1, 1, sizeof(unsigned char) * nsize)),
        DVBT_HIP_CORE_INIT(bit_inner_interleaver, bit_inner_interleaver_params(nsize, constellation, hierarchy, transmission))
    {
    }

  } /* namespace dvbt */
} /* namespace gr */
