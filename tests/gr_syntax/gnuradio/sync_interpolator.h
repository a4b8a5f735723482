/* syntax-check scaffolding only (tests/gr_syntax/README.md): gr::sync_block and gr::sync_interpolator as the convolutional_interleaver shell uses them,
 * declared, not defined */
#ifndef GRSYN_SYNC_INTERPOLATOR_H
#define GRSYN_SYNC_INTERPOLATOR_H
#include <gnuradio/block.h>
namespace gr {
  class sync_block : public block {
  public:
    virtual int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items) = 0;
  protected:
    sync_block();
    sync_block(const std::string &name, io_signature::sptr input_signature, io_signature::sptr output_signature);
  };
  class sync_interpolator : public sync_block {
  public:
    unsigned interpolation() const;
    void set_interpolation(unsigned interpolation);
  protected:
    sync_interpolator();
    sync_interpolator(const std::string &name, io_signature::sptr input_signature, io_signature::sptr output_signature, unsigned interpolation);
  };
}
#endif
