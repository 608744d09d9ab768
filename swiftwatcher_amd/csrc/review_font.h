// The review labels' font (swk_render_review_labels, include/swk.h): 5 x 7 glyphs, one byte per row, bit 4 the leftmost column,
// row 7 = 1 for a byte of the character set; bytes kReviewFontFirst (space) .. 'Z'.  Drawn by hand for this library.
// One initialiser for the host's table (review_plan.cpp) and the kernels' __constant__ copy (review.hip); whoever includes this
// takes the rows and then #undefs SWK_REVIEW_FONT_ROWS, NONE and G.
#define G(a, b, c, d, e, f, g) {0x##a, 0x##b, 0x##c, 0x##d, 0x##e, 0x##f, 0x##g, 1}
#define NONE {0, 0, 0, 0, 0, 0, 0, 0}
#define SWK_REVIEW_FONT_ROWS {                                                                                                  \
    /* space ! " # */ G(00, 00, 00, 00, 00, 00, 00), NONE, NONE, G(0A, 0A, 1F, 0A, 1F, 0A, 0A),                                 \
    /* $ % & ' */     NONE, G(19, 19, 02, 04, 08, 13, 13), NONE, NONE,                                                          \
    /* ( ) * + */     NONE, NONE, NONE, G(00, 04, 04, 1F, 04, 04, 00),                                                          \
    /* , - . / */     NONE, G(00, 00, 00, 1F, 00, 00, 00), G(00, 00, 00, 00, 00, 0C, 0C), G(01, 01, 02, 04, 08, 10, 10),        \
    /* 0 1 2 */       G(0E, 11, 13, 15, 19, 11, 0E), G(04, 0C, 04, 04, 04, 04, 0E), G(0E, 11, 01, 02, 04, 08, 1F),              \
    /* 3 4 5 */       G(1F, 02, 04, 02, 01, 11, 0E), G(02, 06, 0A, 12, 1F, 02, 02), G(1F, 10, 1E, 01, 01, 11, 0E),              \
    /* 6 7 8 */       G(06, 08, 10, 1E, 11, 11, 0E), G(1F, 01, 02, 04, 08, 08, 08), G(0E, 11, 11, 0E, 11, 11, 0E),              \
    /* 9 : ; */       G(0E, 11, 11, 0F, 01, 02, 0C), G(00, 0C, 0C, 00, 0C, 0C, 00), NONE,                                       \
    /* < = > ? @ */   NONE, G(00, 00, 1F, 00, 1F, 00, 00), NONE, NONE, NONE,                                                    \
    /* A B C */       G(0E, 11, 11, 1F, 11, 11, 11), G(1E, 11, 11, 1E, 11, 11, 1E), G(0E, 11, 10, 10, 10, 11, 0E),              \
    /* D E F */       G(1C, 12, 11, 11, 11, 12, 1C), G(1F, 10, 10, 1E, 10, 10, 1F), G(1F, 10, 10, 1E, 10, 10, 10),              \
    /* G H I */       G(0E, 11, 10, 17, 11, 11, 0F), G(11, 11, 11, 1F, 11, 11, 11), G(0E, 04, 04, 04, 04, 04, 0E),              \
    /* J K L */       G(07, 02, 02, 02, 02, 12, 0C), G(11, 12, 14, 18, 14, 12, 11), G(10, 10, 10, 10, 10, 10, 1F),              \
    /* M N O */       G(11, 1B, 15, 15, 11, 11, 11), G(11, 11, 19, 15, 13, 11, 11), G(0E, 11, 11, 11, 11, 11, 0E),              \
    /* P Q R */       G(1E, 11, 11, 1E, 10, 10, 10), G(0E, 11, 11, 11, 15, 12, 0D), G(1E, 11, 11, 1E, 14, 12, 11),              \
    /* S T U */       G(0F, 10, 10, 0E, 01, 01, 1E), G(1F, 04, 04, 04, 04, 04, 04), G(11, 11, 11, 11, 11, 11, 0E),              \
    /* V W X */       G(11, 11, 11, 11, 11, 0A, 04), G(11, 11, 11, 15, 15, 15, 0A), G(11, 11, 0A, 04, 0A, 11, 11),              \
    /* Y Z */         G(11, 11, 11, 0A, 04, 04, 04), G(1F, 01, 02, 04, 08, 10, 1F)}
