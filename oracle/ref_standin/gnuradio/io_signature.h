/* Stand-in for gr::io_signature: records what make() was given. */
#ifndef REF_STANDIN_GR_IO_SIGNATURE_H
#define REF_STANDIN_GR_IO_SIGNATURE_H
#include <gnuradio/types.h>

namespace gr {
  class io_signature {
  public:
    typedef std::shared_ptr<io_signature> sptr;
    int d_min, d_max, d_itemsize;
    static sptr make(int min_streams, int max_streams, int sizeof_stream_item)
    {
      return sptr(new io_signature{min_streams, max_streams, sizeof_stream_item});
    }
    int min_streams() const { return d_min; }
    int max_streams() const { return d_max; }
    int sizeof_stream_item(int) const { return d_itemsize; }
  };
}
#endif
