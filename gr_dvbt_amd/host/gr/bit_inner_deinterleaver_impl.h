/* bit_inner_deinterleaver_impl.h -- HIP-backed body of gr::dvbt::bit_inner_deinterleaver (replaces lib/bit_inner_deinterleaver_impl.h of gr-dvbt; see hip_shell.h) */
#ifndef INCLUDED_DVBT_BIT_INNER_DEINTERLEAVER_IMPL_HIP_H
#define INCLUDED_DVBT_BIT_INNER_DEINTERLEAVER_IMPL_HIP_H

#include <dvbt/bit_inner_deinterleaver.h>
#include "hip_shell.h"

namespace gr {
  namespace dvbt {

    class bit_inner_deinterleaver_impl : public bit_inner_deinterleaver
    {
      hip::core< ::dvbt_bit_inner_deinterleaver, ::dvbt_bit_inner_deinterleaver_params> d_core;
      bool d_hier;                                         /* hierarchy != NH: the second output exists */
    public:
      void forecast(int noutput_items, gr_vector_int &ninput_items_required) { d_core.forecast(noutput_items, ninput_items_required); }
      int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items);

      bit_inner_deinterleaver_impl(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission);
      ~bit_inner_deinterleaver_impl() {}
    };

  } // namespace dvbt
} // namespace gr

#endif
