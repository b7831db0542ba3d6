# map_batch.rb -- the batched calls of Blurrily::Map, over RawMap#find_batch (ruby/ext/blurrily/map_ext_batch.c).
#
#   require 'blurrily/map'
#   require 'blurrily/map_batch'
#
# Counterpart of lib/blurrily/map.rb:8-36 (mezis/blurrily v1.0.2) for batches: the same normalisation, defaults
# and clean-path rule, applied per element, so that
#
#   map.find_batch(needles, limit)[i] == map.find(needles[i], limit)        for every i
#
# (blurrily_amd/map.py is this file's Python mirror and is what tests/ exercise: there is no Ruby in the image
# this repository is built in.)
require 'blurrily/map'

module Blurrily
  class Map < RawMap

    # One GPU batch instead of needles.size finds.  ASCII needles travel as they are and are normalised ON THE
    # DEVICE (blurrily_storage_find_batch_raw: map.rb:40-47 for ASCII input); a needle with a byte >= 0x80
    # needs ActiveSupport's NFKD tables and is normalised here first -- normalize_string is idempotent on its
    # own output, so the device step leaves it alone.
    def find_batch(needles, limit = LIMIT_DEFAULT)
      prepared = needles.map { |n| n.ascii_only? ? n : normalize_string(n) }
      rows, _non_ascii = find_batch_raw(prepared, limit)
      rows
    end

    # needles.size puts in one FFI crossing (weights default to 0, i.e. the string's length: map.rb:9,
    # storage.c:409).  Returns the number of trigrams added.
    def put_batch(needles, references, weights = nil)
      @clean_path = nil
      put_many(needles.map { |n| normalize_string(n) }, references, weights)
    end

    # The best rows of the normalised needle by trigram Jaccard similarity at or above min_permille / 1000:
    # [[ref, matches, weight, R], ...], R the reference's distinct trigrams (RawMap#find_similar; limit <= 0 means
    # LIMIT_DEFAULT, as for find).
    def find_similar(needle, limit = LIMIT_DEFAULT, min_permille = 0)
      super(normalize_string(needle), limit, min_permille)
    end

    # Replicate the device image on the first `n` visible GPUs and shard every later find_batch over them
    # (include/blurrily_storage.h, "devices").  The answer does not depend on n.
    def devices=(n)
      set_option('devices', n)
    end

    def devices
      get_option('devices')
    end
  end
end
