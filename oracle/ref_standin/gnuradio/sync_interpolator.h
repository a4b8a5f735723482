/* Stand-in for gr::sync_interpolator: a block with work() that consumes noutput_items / interpolation per call. */
#ifndef REF_STANDIN_GR_SYNC_INTERPOLATOR_H
#define REF_STANDIN_GR_SYNC_INTERPOLATOR_H
#include <gnuradio/block.h>

namespace gr {
  class sync_interpolator : public block {
  public:
    virtual int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items) = 0;

    void forecast(int noutput_items, gr_vector_int &ninput_items_required)
    {
      for (size_t i = 0; i < ninput_items_required.size(); i++)
        ninput_items_required[i] = noutput_items / si_interpolation;
    }
    int general_work(int noutput_items, gr_vector_int &, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items)
    {
      int r = work(noutput_items, input_items, output_items);
      if (r > 0) consume_each(r / si_interpolation);
      return r;
    }
    unsigned interpolation() const { return si_interpolation; }

    unsigned si_interpolation = 1;

  protected:
    sync_interpolator() {}
    sync_interpolator(const std::string &name, io_signature::sptr in, io_signature::sptr out, unsigned interpolation)
      : block(name, in, out), si_interpolation(interpolation)
    {
      set_output_multiple(interpolation);
      set_relative_rate((double)interpolation);
    }
  };
}
#endif
