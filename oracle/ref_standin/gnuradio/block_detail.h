/* Stand-in for gr::block_detail: the readers of a block's inputs, one per input. */
#ifndef REF_STANDIN_GR_BLOCK_DETAIL_H
#define REF_STANDIN_GR_BLOCK_DETAIL_H
#include <gnuradio/buffer.h>

namespace gr {
  class block_detail {
  public:
    explicit block_detail(unsigned int ninputs)
    {
      for (unsigned int i = 0; i < ninputs; i++) si_inputs.push_back(buffer_reader_sptr(new buffer_reader));
    }
    int ninputs() const { return (int)si_inputs.size(); }
    buffer_reader_sptr input(unsigned int which) { return si_inputs.at(which); }

    std::vector<buffer_reader_sptr> si_inputs;
  };
  typedef std::shared_ptr<block_detail> block_detail_sptr;
}
#endif
