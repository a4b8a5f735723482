/* inner_coder_impl.cc -- gr::dvbt::inner_coder on libdvbt_hip (replaces lib/inner_coder_impl.cc).  ninput must be 1 and noutput a multiple of 1512 (include/dvbt_hip.h T4). */
#include "inner_coder_impl.h"

namespace gr {
  namespace dvbt {

    inner_coder::sptr
    inner_coder::make(int ninput, int noutput, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_code_rate_t coderate)
    { return gnuradio::get_initial_sptr(new inner_coder_impl(ninput, noutput, constellation, hierarchy, coderate)); }

    static dvbt_inner_coder_params inner_coder_params(int ninput, int noutput, int constellation, int hierarchy, int coderate)
    { dvbt_inner_coder_params q = { ninput, noutput, constellation, hierarchy, coderate }; return q; }

    /* io signatures and scheduler hints: lib/inner_coder_impl.cc:133-172 */
    inner_coder_impl::inner_coder_impl(int ninput, int noutput, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_code_rate_t coderate)
      : block("inner_coder", io_signature::make(1, 1, sizeof(unsigned char)), io_signature::make(1, 1, sizeof(unsigned char) * noutput)),
        DVBT_HIP_CORE_INIT(inner_coder, inner_coder_params(ninput, noutput, constellation, hierarchy, coderate))
    {
      set_output_multiple(4);
      /* items out per byte in: 8 n / (k m) coded symbols of every byte, noutput of them to an item.  The reference's expression (:176) multiplies by k m
       * where this divides (0.042 instead of 0.0026 for 16-QAM 1/2); the scheduler sizes buffers and places propagated tags by it */
      dvbt_dims d;
      if (dvbt_get_dims((int)constellation, (int)hierarchy, (int)coderate, 0, 0, &d) < 0) throw std::runtime_error(dvbt_last_error());
      set_relative_rate((double)(ninput * 8 * d.cr_n) / (double)(noutput * d.cr_k * d.m));
    }

  } /* namespace dvbt */
} /* namespace gr */
