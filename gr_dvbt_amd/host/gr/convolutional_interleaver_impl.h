/* convolutional_interleaver_impl.h -- HIP-backed body of gr::dvbt::convolutional_interleaver (replaces lib/convolutional_interleaver_impl.h of gr-dvbt;
 * see hip_shell.h).  A sync_interpolator: the runtime consumes noutput_items / (I * blocks) items itself, so work() passes the call to the C ABI
 * without the consume_each of hip::core::work. */
#ifndef INCLUDED_DVBT_CONVOLUTIONAL_INTERLEAVER_IMPL_HIP_H
#define INCLUDED_DVBT_CONVOLUTIONAL_INTERLEAVER_IMPL_HIP_H

#include <dvbt/convolutional_interleaver.h>
#include "hip_shell.h"

namespace gr {
  namespace dvbt {

    class convolutional_interleaver_impl : public convolutional_interleaver
    {
      ::dvbt_convolutional_interleaver *d_h;
      convolutional_interleaver_impl(const convolutional_interleaver_impl &);
      convolutional_interleaver_impl &operator=(const convolutional_interleaver_impl &);
    public:
      convolutional_interleaver_impl(int blocks, int I, int M);
      ~convolutional_interleaver_impl();
      int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items);
    };

  } // namespace dvbt
} // namespace gr

#endif
