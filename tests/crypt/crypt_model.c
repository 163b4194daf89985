/* Zip.CRC_Crypto's cipher restated literally and byte-serially from the Ada (zip-crc_crypto.adb:31-60, 90-128):
 * the CPU model the GPU path is compared with.  It shares no code with the product library. */
#include <stdint.h>

static uint32_t table[256];
static int table_ready = 0;

static void prepare_table(void) {                       /* Prepare_table :31-47 */
  const uint32_t seed = 0xEDB88320u;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t l = i;
    for (int bit = 0; bit < 8; bit++) {
      if ((l & 1) == 0) l = l >> 1;
      else l = (l >> 1) ^ seed;
    }
    table[i] = l;
  }
  table_ready = 1;
}

static void update(uint32_t *crc, uint8_t by) {         /* Update :49-60, one byte */
  if (!table_ready) prepare_table();
  *crc = table[(*crc & 0xFF) ^ by] ^ (*crc >> 8);
}

static void update_keys(uint32_t keys[3], uint8_t by) { /* Update_keys :90-99 */
  update(&keys[0], by);
  keys[1] = keys[1] + (keys[0] & 0x000000ffu);
  keys[1] = keys[1] * 134775813u + 1u;
  update(&keys[2], (uint8_t)(keys[1] >> 24));
}

static uint8_t crypto_code(const uint32_t keys[3]) {    /* Crypto_code :102-108 */
  uint16_t temp = (uint16_t)((keys[2] & 0xffffu) | 2u);
  return (uint8_t)((uint16_t)(temp * (uint16_t)(temp ^ 1u)) >> 8);
}

void cm_init_keys(const uint8_t *password, uint64_t len, uint32_t keys[3]) {   /* Init_Keys :110-116 */
  keys[0] = 0x12345678u; keys[1] = 0x23456789u; keys[2] = 0x34567890u;
  for (uint64_t i = 0; i < len; i++) update_keys(keys, password[i]);
}

void cm_encode(uint32_t keys[3], uint8_t *buf, uint64_t n) {                   /* Encode :118-128 (mode = encrypted) */
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t bc = buf[i];
    buf[i] = bc ^ crypto_code(keys);
    update_keys(keys, bc);                              /* keys are updated with the unencrypted byte */
  }
}
