/* Stand-in for gr::buffer_reader: what a block can ask about one of its inputs -- whether the block upstream has finished, and how many
 * items wait unread.  Both are whatever the driver set (si_*): there is no buffer. */
#ifndef REF_STANDIN_GR_BUFFER_H
#define REF_STANDIN_GR_BUFFER_H
#include <gnuradio/types.h>

namespace gr {
  class buffer_reader {
  public:
    bool done() const { return si_done; }
    int items_available() const { return si_items; }

    bool si_done = false;
    int si_items = 0;
  };
  typedef std::shared_ptr<buffer_reader> buffer_reader_sptr;
}
#endif
