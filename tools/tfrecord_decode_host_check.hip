// Host-side check of td_tfrecord_decode (csrc/ingest.hip) under the address and undefined-behaviour sanitizers: the
// route predicate over every stride, the CRC tables, the decoder's table builder and the entry's argument checks.
// Nothing here touches a GPU: the entry returns before its first runtime call in every case below.  ingest.hip is
// compiled into this program, and the three functions of api.hip it calls are replaced by recording stubs.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Itelluride_decoding_amd/csrc \
//     tools/tfrecord_decode_host_check.hip -o tools/micro/tfrecord_decode_host_check
//   tools/micro/tfrecord_decode_host_check            (prints "ok" and exits 0)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../telluride_decoding_amd/csrc/ingest.hip"

static std::string g_message;
static int g_uploads = 0;

int td_fail(td_handle*, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_message = buf;
  return code;
}
int td_table_upload(td_handle*, const void*, size_t, const void** dev) {
  ++g_uploads;
  *dev = nullptr;
  return TD_ERR_STATE;
}
int td_scratch(td_handle*, size_t, void** out) {
  *out = nullptr;
  return TD_ERR_STATE;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static uint32_t crc_bytes(const uint8_t* p, size_t n, uint32_t c) {
  const CrcTables& ct = crc_tables();
  for (size_t i = 0; i < n; ++i) c = ct.byte_tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c;
}

static uint32_t advance(const std::vector<uint32_t>& adv, uint32_t c) {
  return adv[c & 0xff] ^ adv[256 + ((c >> 8) & 0xff)] ^ adv[512 + ((c >> 16) & 0xff)] ^ adv[768 + (c >> 24)];
}

int main() {
  // the route: a staged group starts 16-byte aligned and fits the staging area; the CRC pieces tile the data
  for (int stride = 17; stride <= 70000; ++stride) {
    int staged = -1, group = -1, lanes = -1;
    CHECK(td_tfrecord_route(stride, &staged, &group, &lanes) == TD_OK);
    CHECK(lanes >= 1 && lanes <= kThreads);
    if (staged) {
      CHECK(group >= 1 && (long long)group * stride % 16 == 0 && group * stride <= kStageBytes);
      CHECK(group * lanes <= kThreads);
    } else {
      CHECK(group == 0 && lanes == kThreads);
    }
    const int piece = (stride - 16) / lanes;
    CHECK((stride - 16) - (lanes - 1) * piece >= 0);
  }
  CHECK(td_tfrecord_route(16, nullptr, nullptr, nullptr) == TD_ERR_INVALID);

  // CRC-32C ("123456789" -> e3069283) and the split the kernels use: pieces from zero, advanced and xored
  CHECK((crc_bytes(reinterpret_cast<const uint8_t*>("123456789"), 9, 0xffffffffu) ^ 0xffffffffu) == 0xe3069283u);
  std::vector<uint8_t> data(5000);
  for (size_t i = 0; i < data.size(); ++i) data[i] = (uint8_t)(i * 131 + (i >> 3));
  for (int lanes : {1, 4, 8, 256}) {
    const int len = (int)data.size(), piece = len / lanes, first = len - (lanes - 1) * piece;
    const std::vector<uint32_t>& adv = crc_tables().advance_by(piece);
    uint32_t c = crc_bytes(data.data(), first, 0xffffffffu);
    for (int k = 1; k < lanes; ++k) c = advance(adv, c) ^ crc_bytes(data.data() + first + (k - 1) * piece, piece, 0u);
    CHECK(c == crc_bytes(data.data(), data.size(), 0xffffffffu));
  }

  // the table builder, on both sides of the route predicate
  for (int stride : {17, 318, 650, 16423, 49152, 49153, 80044}) {
    std::vector<uint8_t> tmpl(stride), mask(stride, 1);
    const uint64_t length = (uint64_t)stride - 16;
    for (int b = 0; b < stride; ++b) tmpl[b] = (uint8_t)(b * 7 + 1);
    memcpy(tmpl.data(), &length, 8);
    for (int b = stride - 4; b < stride; ++b) mask[b] = 0;
    mask[12] = 0;
    int staged, group, lanes;
    CHECK(td_tfrecord_route(stride, &staged, &group, &lanes) == TD_OK);
    std::vector<uint32_t> tab;
    decode_table(tmpl.data(), mask.data(), stride, (stride - 16) / lanes, &tab);
    CHECK(tab.size() == (size_t)kTabWords + 2 * (size_t)stride);
    const uint8_t* t4 = reinterpret_cast<const uint8_t*>(tab.data() + kTabWords);
    const uint8_t* m4 = t4 + 4 * (size_t)stride;
    for (size_t b = 0; b < 4 * (size_t)stride; ++b) {
      CHECK(t4[b] == tmpl[b % stride]);
      CHECK(m4[b] == (mask[b % stride] ? 0xff : 0x00));
    }

    // the entry's argument checks; `h` is never dereferenced before the table upload (the stub above)
    alignas(16) static unsigned char handle_bytes[64];
    td_handle* h = reinterpret_cast<td_handle*>(handle_bytes);
    alignas(16) static uint8_t image[64];
    alignas(8) static int64_t status[1];
    alignas(4) static float dst[64];
    void* dsts[17];
    int offs[17], counts[17], cols[17];
    int64_t lds[17];
    for (int o = 0; o < 17; ++o) { dsts[o] = dst; offs[o] = 13; counts[o] = 1; cols[o] = 2; lds[o] = 3; }
    auto call = [&](const uint8_t* img, int s, int64_t frames, const uint8_t* t, const uint8_t* m, int n, int64_t* st) {
      g_message.clear();
      return td_tfrecord_decode(h, img, s, frames, t, m, n, offs, counts, dsts, lds, cols, st);
    };
    if (stride < 21) continue;                                    // (no room for a payload)
    CHECK(call(image, stride, 0, tmpl.data(), mask.data(), 16, status) == TD_OK);                // frames == 0
    CHECK(call(nullptr, stride, 0, tmpl.data(), mask.data(), 0, status) == TD_OK);
    const int uploads = g_uploads;
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_STATE && g_uploads == uploads + 1);
    CHECK(call(nullptr, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(g_message.find("NULL") != std::string::npos);
    CHECK(call(image, stride, 1, nullptr, mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(call(image, stride, 1, tmpl.data(), nullptr, 1, status) == TD_ERR_INVALID);
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, nullptr) == TD_ERR_INVALID);
    CHECK(td_tfrecord_decode(nullptr, image, stride, 1, tmpl.data(), mask.data(), 0, offs, counts, dsts, lds, cols,
                             status) == TD_ERR_INVALID);
    CHECK(call(image, 16, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(call(image, stride, -1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(call(image, stride + 1, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(g_message.find("length field") != std::string::npos);
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 17, status) == TD_ERR_INVALID);
    CHECK(g_message.find("outputs") != std::string::npos);
    CHECK(call(image + 4, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(g_message.find("aligned") != std::string::npos);
    offs[0] = 11;
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(g_message.find("outside") != std::string::npos);
    offs[0] = stride - 7;                                         // the last byte of the payload is a CRC byte
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    offs[0] = stride - 8;
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_STATE);
    offs[0] = 13;
    lds[0] = 2;                                                   // column 2 + 1 float needs a row stride of 3
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    CHECK(g_message.find("row stride") != std::string::npos);
    lds[0] = 3;
    dsts[0] = nullptr;
    CHECK(call(image, stride, 1, tmpl.data(), mask.data(), 1, status) == TD_ERR_INVALID);
    dsts[0] = dst;
    CHECK(g_uploads == uploads + 2);
  }
  printf("ok\n");
  return 0;
}
