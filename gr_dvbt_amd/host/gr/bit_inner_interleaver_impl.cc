/* bit_inner_interleaver_impl.cc -- gr::dvbt::bit_inner_interleaver on libdvbt_hip (replaces lib/bit_inner_interleaver_impl.cc).  
 * Non-hierarchical only: hierarchy != NH is refused (include/dvbt_hip.h T5), so the block declares ONE input where the reference declares (1, 2): the reference's
 * second input carries the low-priority stream of a hierarchical transmission and is never read otherwise (:127-176), and its forecast asks for as much of it
 * as of the first.  A flowgraph that connects a second input is refused when it is built, not left waiting for items nobody reads. */
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
