/* convolutional_interleaver_impl.cc -- gr::dvbt::convolutional_interleaver on libdvbt_hip (replaces lib/convolutional_interleaver_impl.cc).
 * out[t] = x[t - I*M*(t mod I)] for any I and M; the last (I-1)*M*I input bytes stay on the device between calls. */
#include "convolutional_interleaver_impl.h"

namespace gr {
  namespace dvbt {

    convolutional_interleaver::sptr
    convolutional_interleaver::make(int nsize, int I, int M)
    { return gnuradio::get_initial_sptr(new convolutional_interleaver_impl(nsize, I, M)); }

    /* io signatures and interpolation: lib/convolutional_interleaver_impl.cc:44-48 */
    convolutional_interleaver_impl::convolutional_interleaver_impl(int blocks, int I, int M)
      : sync_interpolator("convolutional_interleaver", io_signature::make(1, 1, sizeof(unsigned char) * I * blocks),
                          io_signature::make(1, 1, sizeof(unsigned char)), I * blocks),
        d_h(0)
    {
      dvbt_convolutional_interleaver_params p = { blocks, I, M };
      if (dvbt_convolutional_interleaver_create(&p, &d_h) < 0)        /* no CPU fallback */
        throw std::runtime_error(std::string("libdvbt_hip: ") + dvbt_last_error());
    }

    convolutional_interleaver_impl::~convolutional_interleaver_impl() { if (d_h) dvbt_convolutional_interleaver_destroy(d_h); }

    int
    convolutional_interleaver_impl::work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items)
    {
      const int n = dvbt_convolutional_interleaver_work(d_h, noutput_items, noutput_items / (int)interpolation(), input_items[0], output_items[0], 0);
      if (n < 0) throw std::runtime_error(std::string("libdvbt_hip: ") + dvbt_last_error());
      return n;
    }

  } /* namespace dvbt */
} /* namespace gr */
