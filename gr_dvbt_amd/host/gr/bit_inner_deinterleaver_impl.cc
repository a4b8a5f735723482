/* bit_inner_deinterleaver_impl.cc -- gr::dvbt::bit_inner_deinterleaver on libdvbt_hip (replaces lib/bit_inner_deinterleaver_impl.cc).
 * Non-hierarchical modes: one output stream, the second output of :73-75 is not written (as in the reference).  Hierarchical modes (ALPHA1 / 2 / 4):
 * the high-priority bytes on output 0 and the low-priority bytes on output 1 through dvbt_bit_inner_deinterleaver_work_hier; a flowgraph that connects
 * output 0 alone gets it from dvbt_bit_inner_deinterleaver_work.  The library rejects hierarchical QPSK (include/dvbt_hip.h A6). */
#include "bit_inner_deinterleaver_impl.h"

namespace gr {
  namespace dvbt {

    bit_inner_deinterleaver::sptr
    bit_inner_deinterleaver::make(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission)
    { return gnuradio::get_initial_sptr(new bit_inner_deinterleaver_impl(nsize, constellation, hierarchy, transmission)); }

    static dvbt_bit_inner_deinterleaver_params bit_params(int nsize, int c, int h, int t)
    { dvbt_bit_inner_deinterleaver_params p = { nsize, c, h, t }; return p; }

    /* io signatures: lib/bit_inner_deinterleaver_impl.cc:73-75 */
    bit_inner_deinterleaver_impl::bit_inner_deinterleaver_impl(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy,
                                                               dvbt_transmission_mode_t transmission)
      : block("bit_inner_deinterleaver", io_signature::make(1, 1, sizeof(unsigned char) * nsize), io_signature::make(1, 2, sizeof(unsigned char) * nsize)),
        DVBT_HIP_CORE_INIT(bit_inner_deinterleaver, bit_params(nsize, (int)constellation, (int)hierarchy, (int)transmission)),
        d_hier(hierarchy != NH)
    {
    }

    namespace {
      struct call_work_hier {
        ::dvbt_bit_inner_deinterleaver *h; int noutput_items, ninput_items; const void *in; void *hp, *lp;
        int operator()(dvbt_sideband *sb) const { return ::dvbt_bit_inner_deinterleaver_work_hier(h, noutput_items, ninput_items, in, hp, lp, sb); }
      };
    }

    int
    bit_inner_deinterleaver_impl::general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &input_items,
                                               gr_vector_void_star &output_items)
    {
      if (!d_hier || output_items.size() < 2)
        return d_core.work(this, noutput_items, ninput_items[0], input_items[0], output_items[0]);
      call_work_hier c = { d_core.handle(), noutput_items, ninput_items[0], input_items[0], output_items[0], output_items[1] };
      return d_core.work_with(this, ninput_items[0], c);
    }

  } /* namespace dvbt */
} /* namespace gr */
